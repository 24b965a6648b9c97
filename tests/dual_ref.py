"""The definition of dual contouring of the field, in plain NumPy over an evaluator `ev(P) -> (N,) float64`:
what csrc/sdf_dual.hip reproduces bit for bit.  Ju, Losasso, Schaefer, Warren 2002: one vertex in every grid cell that the surface
crosses, placed by the quadric of the tangent planes at the cell's edge crossings, one quad per crossing edge.  Every float64
operation below is one IEEE operation, in the order written; nothing is fused.

Input: the axes X (nx), Y (ny), Z (nz) float64 as `core.grid_axes` returns them, eps > 0 (the step of the normals' central
difference), reg >= 0.

Samples.  V[i, j, k] = ev((X[i], Y[j], Z[k])), the linear index of a sample is s = (i * ny + j) * nz + k, inside = V < 0 (so 0.0,
-0.0 and NaN are not inside).

Crossing edges.  The edge (s, a) runs from sample s to its +1 neighbour along axis a.  It is a crossing if both values are finite
and `inside` differs at its ends; an edge whose ends differ in `inside` but which has a non-finite end is counted in
`nonfinite_edges` and otherwise ignored.  The crossings are numbered by ascending (s, a).  With lo, hi the axis values at the two ends
and v0, v1 the samples: t = v0 / (v0 - v1), p[a] = lo + t * (hi - lo), the other two coordinates are the axis values themselves.
The normal n of a crossing is `normals_ref.vertex_normals(ev, p, eps)`: the zero vector where the field is flat.

Cells.  Cell (i, j, k), 0 <= i < nx - 1 and likewise, linear index in C order over (nx - 1, ny - 1, nz - 1); centre
c_a = lo_a + 0.5 * (hi_a - lo_a), half size h_a = 0.5 * (hi_a - lo_a).  Its twelve edges in this order: for a in 0, 1, 2, for
(db, dc) in (0, 0), (1, 0), (0, 1), (1, 1) with b = (a + 1) % 3, c = (a + 2) % 3: the edge along a whose low end is the cell's corner
moved by db along b and dc along c.  Over the crossings among them, in that order, from 0.0 and left to right: the count, the sum
of q = p - centre, the six sums n_i * n_j (i <= j), the three sums n_i * d with d = (n0 * q0 + n1 * q1) + n2 * q2.  A cell with a
count > 0 is active; m = sum_q / count.

Vertex (`solve`).  The system of `simplify_ref.solve`: w = (A00 + A11) + A22, lam = reg * w, g = b - A m, y by cofactors over the
determinant, x = m + y.  w == 0 gives x = m (`flat`); else a non-finite component gives x = m (`mean_fallback`); else every component
is clamped to [-h_a, h_a] by np.minimum(np.maximum(x, -h), h), and a cell where that changed a component counts as `clamped`.
v = centre + x.  Active cells are numbered by ascending linear index: that is the vertex array, without duplicates by construction.

Triangles.  For every crossing, in crossing order, the four cells round it: with the low end at cell coordinates (.., ib, ic), the
cells at offsets (-1, -1), (0, -1), (0, 0), (-1, 0) in (b, c), q0 .. q3.  If one of them does not exist (the edge lies on the grid's
border) the crossing emits nothing and counts in `open_edges`.  If the low end is not inside the order is reversed (q3 .. q0).  Two
triangles: (q0, q1, q2), (q0, q2, q3).

Refusals (ValueError before any output): nx * ny * nz >= 2^31, eps not positive and finite, reg negative or not finite, an axis that is
not finite.  An axis of fewer than 2 samples gives the empty mesh."""
import collections

import numpy as np

import normals_ref

Dual = collections.namedtuple('Dual', ('vertices', 'cells', 'soup', 'stats', 'points', 'normals', 'edges', 'active'))
Dual.__doc__ = """vertices (K, 3) float64, cells (T, 3) int64, soup (T, 3, 3) float64 = vertices[cells], stats (dict of the integers
STAT_KEYS): what the device reproduces, and points (C, 3), normals (C, 3) of the crossings.  For the tests: edges (C, 2) int64 the
(s, a) of the crossings, active (K,) int64 the linear indices of the active cells."""

STAT_KEYS = ('crossings', 'cells', 'triangles', 'open_edges', 'nonfinite_edges', 'clamped', 'mean_fallback', 'flat')
QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))                # the four cells round an edge, as offsets in (b, c)
EDGES = tuple((a, db, dc) for a in range(3) for db, dc in ((0, 0), (1, 0), (0, 1), (1, 1)))      # the twelve edges of a cell


def check_args(X, Y, Z, eps, reg):
    """(X, Y, Z, eps, reg) as float64, or ValueError"""
    axes = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (X, Y, Z)]
    eps, reg = float(eps), float(reg)
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError('dual: eps must be positive and finite, got %r' % (eps,))
    if not (np.isfinite(reg) and reg >= 0):
        raise ValueError('dual: reg must be finite and not negative, got %r' % (reg,))
    for name, a in zip('XYZ', axes):
        if not np.isfinite(a).all():
            raise ValueError('dual: axis %s is not finite' % name)
    if len(axes[0]) * len(axes[1]) * len(axes[2]) >= 2 ** 31:
        raise ValueError('dual: 2^31 or more samples')
    return axes[0], axes[1], axes[2], eps, reg


def solve(quadric, mean, half, reg):
    """(x (K, 3), flat, fallback, clamped (K,) bool): the vertex about the centre of its cell, one operation per line -- the system of
    simplify_ref.solve, then clamping in the place of its mean fallback"""
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
        fallback = ~flat & ~np.isfinite(x).all(axis=1)
        xc = np.minimum(np.maximum(x, -half), half)
        clamped = ~flat & ~fallback & (xc != x).any(axis=1)
    x = np.where((flat | fallback)[:, None], mean, xc)
    return x, flat, fallback, clamped


def empty(nonfinite=0):
    stats = dict.fromkeys(STAT_KEYS, 0)
    stats['nonfinite_edges'] = int(nonfinite)
    z3, zi = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)
    return Dual(z3, zi, np.zeros((0, 3, 3), np.float64), stats, z3.copy(), z3.copy(), np.zeros((0, 2), np.int64), np.zeros(0, np.int64))


def dual(ev, X, Y, Z, eps, reg=1e-3):
    """the Dual of the field `ev` on the grid X x Y x Z"""
    X, Y, Z, eps, reg = check_args(X, Y, Z, eps, reg)
    axes = (X, Y, Z)
    n = np.array([len(X), len(Y), len(Z)], np.int64)
    if n.min() < 2:
        return empty()
    stride = np.array([n[1] * n[2], n[2], 1], np.int64)
    G = np.stack(np.meshgrid(X, Y, Z, indexing='ij'), axis=-1).reshape(-1, 3)
    V = np.asarray(ev(np.ascontiguousarray(G)), dtype=np.float64).reshape(tuple(n))
    del G
    inside, finite = V < 0, np.isfinite(V)
    # ---- the crossing edges, numbered by ascending (s, a) ----
    S = np.arange(n.prod(), dtype=np.int64).reshape(tuple(n))
    keys, nonfinite = [], 0
    for a in range(3):
        lo = tuple(slice(0, -1) if k == a else slice(None) for k in range(3))
        hi = tuple(slice(1, None) if k == a else slice(None) for k in range(3))
        differ = inside[lo] != inside[hi]
        both = finite[lo] & finite[hi]
        nonfinite += int((differ & ~both).sum())
        keys.append(S[lo][differ & both] * 4 + a)
    keys = np.sort(np.concatenate(keys))
    es, ea = keys >> 2, keys & 3
    C = len(keys)
    if C == 0:
        return empty(nonfinite)
    edge_id = np.full((int(n.prod()), 3), -1, np.int64)
    edge_id[es, ea] = np.arange(C)
    # ---- their points and normals ----
    idx = np.stack(np.unravel_index(es, tuple(n)), axis=1).astype(np.int64)        # (C, 3): the low end
    P = np.stack([X[idx[:, 0]], Y[idx[:, 1]], Z[idx[:, 2]]], axis=1)
    vflat = V.reshape(-1)
    v0, v1 = vflat[es], vflat[es + stride[ea]]
    with np.errstate(all='ignore'):
        t = v0 / (v0 - v1)
    for a in range(3):
        sel = ea == a
        lo, hi = axes[a][idx[sel, a]], axes[a][idx[sel, a] + 1]
        P[sel, a] = lo + t[sel] * (hi - lo)
    N = normals_ref.vertex_normals(ev, P, eps)[0]
    # ---- the active cells and their sums, the twelve edges in the fixed order ----
    nc = n - 1
    ci = np.stack(np.meshgrid(*(np.arange(k, dtype=np.int64) for k in nc), indexing='ij'), axis=-1).reshape(-1, 3)     # C order
    corner = ci @ stride
    eids = np.empty((len(ci), 12), np.int64)
    for k, (a, db, dc) in enumerate(EDGES):
        b, c = (a + 1) % 3, (a + 2) % 3
        eids[:, k] = edge_id[corner + db * stride[b] + dc * stride[c], a]
    act = np.flatnonzero((eids >= 0).any(axis=1))
    eids, ci = eids[act], ci[act]
    K = len(act)
    lo3 = np.stack([axes[a][ci[:, a]] for a in range(3)], axis=1)
    hi3 = np.stack([axes[a][ci[:, a] + 1] for a in range(3)], axis=1)
    half = 0.5 * (hi3 - lo3)
    centre = lo3 + half
    count = np.zeros(K, np.float64)
    sq = np.zeros((K, 3), np.float64)
    quad = np.zeros((K, 9), np.float64)
    with np.errstate(all='ignore'):
        for k in range(12):
            on = np.flatnonzero(eids[:, k] >= 0)
            e = eids[on, k]
            q = P[e] - centre[on]
            nn = N[e]
            n0, n1, n2 = nn[:, 0], nn[:, 1], nn[:, 2]
            d = (n0 * q[:, 0] + n1 * q[:, 1]) + n2 * q[:, 2]
            count[on] = count[on] + 1.0
            sq[on] = sq[on] + q
            quad[on] = quad[on] + np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, n0 * d, n1 * d, n2 * d], axis=1)
        mean = sq / count[:, None]
    x, flat, fallback, clamped = solve(quad, mean, half, reg)
    vertices = centre + x
    # ---- two triangles per crossing that has its four cells ----
    cell_stride = np.array([nc[1] * nc[2], nc[2], 1], np.int64)
    rank = np.full(int(nc.prod()), -1, np.int64)
    rank[act] = np.arange(K)
    b, c = (ea + 1) % 3, (ea + 2) % 3
    rows = np.arange(C)
    ib, ic = idx[rows, b], idx[rows, c]
    has = (ib >= 1) & (ic >= 1) & (ib <= nc[b] - 1) & (ic <= nc[c] - 1)
    base = idx[rows, ea] * cell_stride[ea]
    q4 = np.stack([base + (ib + ob) * cell_stride[b] + (ic + oc) * cell_stride[c] for ob, oc in QUAD], axis=1)[has]
    q4 = rank[q4]
    assert (q4 >= 0).all()
    q4 = np.where(inside.reshape(-1)[es[has]][:, None], q4, q4[:, ::-1])
    cells = np.stack([q4[:, [0, 1, 2]], q4[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    stats = {'crossings': C, 'cells': K, 'triangles': len(cells), 'open_edges': int(C - has.sum()), 'nonfinite_edges': nonfinite,
             'clamped': int(clamped.sum()), 'mean_fallback': int(fallback.sum()), 'flat': int(flat.sum())}
    return Dual(vertices, cells, vertices[cells], stats, P, N, np.stack([es, ea], axis=1), act)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- what the tests measure on a mesh (vertices, cells) ----

def edge_census(cells):
    """dict: boundary (edges with one face), nonmanifold (edges with more than two), misoriented (edges with two faces that run the
    same way), closed, oriented, euler -- of the indexed mesh `cells` (T, 3) over the vertices it uses"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    he = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]])
    lo, hi = he.min(axis=1), he.max(axis=1)
    sign = np.where(he[:, 0] < he[:, 1], 1, -1)
    key = lo * (cells.max() + 1 if len(cells) else 1) + hi
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    net = np.bincount(inv.reshape(-1), weights=sign, minlength=len(uniq))
    boundary, nonmanifold = int((cnt == 1).sum()), int((cnt > 2).sum())
    misoriented = int(((cnt == 2) & (net != 0)).sum())
    used = len(np.unique(cells))
    return {'boundary': boundary, 'nonmanifold': nonmanifold, 'misoriented': misoriented, 'closed': boundary == 0 and nonmanifold == 0,
            'oriented': misoriented == 0 and bool(((cnt != 2) | (net == 0)).all()), 'euler': used - len(uniq) + len(cells), 'edges': len(uniq)}


def volume(soup):
    s = np.asarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    return float((np.cross(s[:, 0], s[:, 1]) * s[:, 2]).sum() / 6.0)


def deviation(ev, soup):
    """(max, rms) of |f| over the corners, edge midpoints and centroids of the soup (T, 3, 3)"""
    s = np.asarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    a, b, c = s[:, 0], s[:, 1], s[:, 2]
    pts = np.concatenate([a, b, c, 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a), (a + b + c) / 3.0])
    v = np.abs(np.asarray(ev(np.ascontiguousarray(pts)), dtype=np.float64))
    return float(v.max()), float(np.sqrt((v * v).mean()))


def against_gradient(ev, soup, eps=1e-5, min_area=1e-12):
    """(the number of faces of area > min_area whose normal points against the field's gradient at the centroid, the number of such
    faces)"""
    s = np.asarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    fn = np.cross(s[:, 1] - s[:, 0], s[:, 2] - s[:, 0])
    area = 0.5 * np.sqrt((fn * fn).sum(axis=1))
    big = area > min_area
    cen = s.sum(axis=1) / 3.0
    g = np.zeros_like(cen)
    for k in range(3):
        d = np.zeros(3)
        d[k] = eps
        g[:, k] = np.asarray(ev(cen + d)) - np.asarray(ev(cen - d))
    return int((((fn * g).sum(axis=1) < 0) & big).sum()), int(big.sum())
