"""The definition of mesh simplification by vertex clustering with quadric vertices, in plain NumPy: what
csrc/sdf_simplify.hip reproduces bit for bit.  Rossignac-Borrel clustering on a uniform grid, one representative per cluster placed
by a quadric error function (Lindstrom's out-of-core simplification).

Input: the weld of a mesh (`Mesh.weld()`: points (U, 3) float64 in welded order, cells (T, 3) int64), `origin` (3,), `cell` (3,)
positive and finite, `reg` >= 0.  Every float64 operation below is one IEEE operation, in the order written; nothing is fused.

Clusters.  fq = floor((p - origin) / cell) per axis, q = int64(fq), qmin the per-axis minimum over the vertices; the key of a vertex
is ((qx - qminx) << 42) | ((qy - qminy) << 21) | (qz - qminz), clusters are numbered 0 .. K - 1 by ascending key, and
centre_k = origin + (q_k + 0.5) * cell.  floor, not truncation: negative coordinates fall into the cell below; -0.0 and +0.0 fall
into the same cell.

Mean.  m_k = (the sum of (p - centre_k) over the cluster's vertices in ascending welded index, left to right, from 0.0) / count.

Quadric.  Every (triangle t, corner c) is item 3t + c of the cluster k of cells[t, c].  With a' = a - centre_k, b' = b - centre_k,
c' = c - centre_k (a, b, c the triangle's three points, all about the centre of the ITEM's cluster): e1 = b' - a', e2 = c' - a',
n = e1 x e2 with every component (u * v) - (w * z), d = (nx * a'x + ny * a'y) + nz * a'z.  The cluster accumulates, from 0.0 and in
ascending item index, the six sums A_ij of n_i * n_j (i <= j) and the three sums b_i of n_i * d: the plane of every triangle that
touches the cluster, weighted by its squared area (|n| is twice the area; Lindstrom's choice -- there is no sqrt).

Representative (`solve`).  w = (A00 + A11) + A22.  w == 0 (`flat`: nothing but zero-area triangles) gives x = m_k.  Otherwise the
system (A + reg w I) x = b + reg w m_k is solved for the offset y = x - m_k, that is (A + reg w I) y = b - A m_k, by cofactors over
the determinant, and x = m_k + y.  (The same system; about the mean the right-hand side of a planar cluster is rounding noise, so
the result stays on the plane to rounding, where the cofactors of the regularised matrix lose reg^-2 of relative accuracy.)  If a
component of x is not finite, or |x_i| > cell_i / 2, x = m_k (`mean_fallback`).  v_k = centre_k + x.  The regularisation makes the
system positive definite for planar and straight-edge clusters (it stands in for Lindstrom's truncated SVD); the fallback keeps a
vertex inside its cell, so the mesh cannot fold through a neighbouring cell.

Triangles.  A triangle survives if its three clusters differ; survivors keep their order and their winding.  The output is the SOUP
of the survivors (T', 3, 3) float64 with v_k at the corners; clusters that no survivor touches appear nowhere in it.  Duplicate
triangles, and oppositely wound pairs where two sheets of the surface fall into the same cells, are NOT removed: the edge census of
`measure` reports them (non-manifold edges).  Topology is not preserved: handles and gaps narrower than a cell close.

Refusals (ValueError, before any output exists): cell not positive and finite, origin not finite, reg negative or not finite; 2^31
or more vertices or corners (3 x triangles: the items are numbered in 31 bits, as the half-edges of the census are); a vertex that
is not finite; an |fq| of 2^53 or more or a per-axis range of q of 2^21 or more."""
import collections

import numpy as np

Simplified = collections.namedtuple('Simplified', ('soup', 'stats', 'vertices', 'vertex_cluster', 'centres', 'means', 'used'))
Simplified.__doc__ = """soup (T', 3, 3) float64 and stats (dict of the integers clusters, triangles_in, triangles_out, collapsed,
mean_fallback, flat): what the device reproduces.  For the tests: vertices (K, 3) the representatives v_k, vertex_cluster (U,) int64,
centres (K, 3), means (K, 3) the m_k, used (K,) bool: a survivor touches the cluster."""

STAT_KEYS = ('clusters', 'triangles_in', 'triangles_out', 'collapsed', 'mean_fallback', 'flat')
KEY_BITS = 21


def check_args(origin, cell, reg):
    """(origin (3,), cell (3,), reg) as float64, or ValueError"""
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    c = np.asarray(cell, dtype=np.float64).reshape(-1)
    if o.shape != (3,) or c.shape != (3,):
        raise ValueError('simplify: origin and cell have 3 components each, got %r and %r' % (origin, cell))
    if not (np.isfinite(c).all() and (c > 0).all()):
        raise ValueError('simplify: cell must be positive and finite, got %r' % (cell,))
    if not np.isfinite(o).all():
        raise ValueError('simplify: origin must be finite, got %r' % (origin,))
    reg = float(reg)
    if not (np.isfinite(reg) and reg >= 0):
        raise ValueError('simplify: reg must be finite and not negative, got %r' % (reg,))
    return o, c, reg


def clusters(points, origin, cell):
    """(vertex_cluster (U,) int64, q (K, 3) int64, centres (K, 3) float64) of finite points; ValueError for a key out of range"""
    if not np.isfinite(points).all():
        raise ValueError('simplify: %d vertices are not finite' % int((~np.isfinite(points).all(axis=1)).sum()))
    if len(points) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float64)
    with np.errstate(over='ignore'):
        fq = np.floor((points - origin) / cell)
    lo, hi = fq.min(axis=0), fq.max(axis=0)
    if not (np.abs(fq) < 2.0 ** 53).all() or ((hi - lo) >= 2.0 ** KEY_BITS).any():
        raise ValueError('simplify: the clusters span 2^%d or more cells on an axis (cell %r is too small for this mesh)' % (KEY_BITS, cell.tolist()))
    q = fq.astype(np.int64)
    rel = q - q.min(axis=0)
    key = (rel[:, 0] << (2 * KEY_BITS)) | (rel[:, 1] << KEY_BITS) | rel[:, 2]
    keys, vertex_cluster = np.unique(key, return_inverse=True)
    qk = np.stack([keys >> (2 * KEY_BITS), (keys >> KEY_BITS) & ((1 << KEY_BITS) - 1), keys & ((1 << KEY_BITS) - 1)], axis=1) + q.min(axis=0)
    centres = origin + (qk.astype(np.float64) + 0.5) * cell
    return np.asarray(vertex_cluster, dtype=np.int64).reshape(-1), qk, centres


def segment_sums(segment, values, n_segments):
    """(n_segments, C) float64: per segment the sum of the rows of values (N, C) whose segment it is, in ascending row index, left to
    right from 0.0 -- one vectorised step per rank inside a segment; and the counts (n_segments,) int64"""
    order = np.argsort(segment, kind='stable')
    counts = np.bincount(segment, minlength=n_segments).astype(np.int64)
    starts = np.cumsum(counts) - counts
    sums = np.zeros((n_segments, values.shape[1]), np.float64)
    live = np.flatnonzero(counts > 0)
    r = 0
    while len(live):
        sums[live] = sums[live] + values[order[starts[live] + r]]
        r += 1
        live = live[counts[live] > r]
    return sums, counts


def means(points, vertex_cluster, centres):
    """m_k (K, 3)"""
    sums, counts = segment_sums(vertex_cluster, points - centres[vertex_cluster], len(centres))
    return sums / counts[:, None].astype(np.float64)


def quadrics(points, cells, vertex_cluster, centres):
    """(K, 9): A00, A01, A02, A11, A12, A22, b0, b1, b2 of every cluster"""
    k = len(centres)
    item_cluster = vertex_cluster[cells].reshape(-1)              # item 3t + c
    c = centres[item_cluster]
    tri = np.repeat(np.arange(len(cells)), 3)
    a = points[cells[tri, 0]] - c
    b = points[cells[tri, 1]] - c
    cc = points[cells[tri, 2]] - c
    e1, e2 = b - a, cc - a
    with np.errstate(all='ignore'):
        nx = (e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1])
        ny = (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2])
        nz = (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])
        d = (nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2]
        terms = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d], axis=1)
        return segment_sums(item_cluster, terms, k)[0]


def solve(quadric, mean, cell, reg):
    """(x (K, 3), flat (K,) bool, fallback (K,) bool): the representative about the centre of its cell, one operation per line"""
    with np.errstate(all='ignore'):
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = (quadric[:, i] for i in range(9))
        m0, m1, m2 = mean[:, 0], mean[:, 1], mean[:, 2]
        w = (a00 + a11) + a22
        lam = reg * w
        g0 = b0 - ((a00 * m0 + a01 * m1) + a02 * m2)
        g1 = b1 - ((a01 * m0 + a11 * m1) + a12 * m2)
        g2 = b2 - ((a02 * m0 + a12 * m1) + a22 * m2)
        d00 = a00 + lam
        d11 = a11 + lam
        d22 = a22 + lam
        c00 = (d11 * d22) - (a12 * a12)
        c01 = (a02 * a12) - (a01 * d22)
        c02 = (a01 * a12) - (a02 * d11)
        c11 = (d00 * d22) - (a02 * a02)
        c12 = (a01 * a02) - (d00 * a12)
        c22 = (d00 * d11) - (a01 * a01)
        det = (d00 * c00 + a01 * c01) + a02 * c02
        y0 = ((c00 * g0 + c01 * g1) + c02 * g2) / det
        y1 = ((c01 * g0 + c11 * g1) + c12 * g2) / det
        y2 = ((c02 * g0 + c12 * g1) + c22 * g2) / det
        x = np.stack([m0 + y0, m1 + y1, m2 + y2], axis=1)
        flat = w == 0
        inside = np.isfinite(x).all(axis=1) & (np.abs(x) <= cell * 0.5).all(axis=1)
    fallback = ~flat & ~inside
    x[flat | fallback] = mean[flat | fallback]
    return x, flat, fallback


def simplify(points, cells, origin, cell, reg=1e-3):
    """the Simplified of the welded mesh (points (U, 3) float64, cells (T, 3) int64) on the grid (origin, cell)"""
    origin, cell, reg = check_args(origin, cell, reg)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    if len(points) >= 2 ** 31 or 3 * len(cells) >= 2 ** 31:
        raise ValueError('simplify: 2^31 or more vertices or corners (3 x triangles)')
    vertex_cluster, qk, centres = clusters(points, origin, cell)
    k = len(centres)
    mean = means(points, vertex_cluster, centres) if k else np.zeros((0, 3))
    quadric = quadrics(points, cells, vertex_cluster, centres) if k else np.zeros((0, 9))
    x, flat, fallback = solve(quadric, mean, cell, reg)
    vertices = centres + x
    tc = vertex_cluster[cells]
    live = (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])
    soup = vertices[tc[live]].reshape(-1, 3, 3)
    used = np.zeros(k, bool)
    used[tc[live].reshape(-1)] = True
    stats = {'clusters': k, 'triangles_in': len(cells), 'triangles_out': int(live.sum()), 'collapsed': int(len(cells) - live.sum()),
             'mean_fallback': int(fallback.sum()), 'flat': int(flat.sum())}
    return Simplified(soup, stats, vertices, vertex_cluster, centres, mean, used)


def weld(soup):
    """(points, cells) of a host soup (T, 3, 3): np.unique over the rows, as `Mesh.weld()` orders them"""
    pts, inv = np.unique(np.asarray(soup, dtype=np.float64).reshape(-1, 3), axis=0, return_inverse=True)
    return pts, np.asarray(inv, dtype=np.int64).reshape(-1, 3)
