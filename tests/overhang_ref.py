"""The definition of a build direction's rating: for a triangle soup and a direction "up" -- the bed lies below
the part -- the area of the faces steeper than the printer's overhang angle, the volume of support under them, the area that lies
on the bed, and the height.  Plain NumPy, float64, one rounding per written operation; no np.dot, `@` or einsum and no np.sum over
the triangles (measure_ref.py says why).  csrc/sdf_overhang.hip (k_overhang_extents, k_overhang_terms, k_overhang_partials,
k_overhang_classes) reproduces `rate` bit for bit; sdf_amd/overhang.py restates `normalise`, `sin_limit_of` and `derive`.

PER TRIANGLE (a, b, c): finite = all nine coordinates are finite; the raw normal n = (b - a) x (c - a) and dbl = |n|, the doubled
area.  PER DIRECTION d (unit length: `normalise`): h(p) = (px dx + py dy) + pz dz; lo, hi = the extremes of h over the vertices of
the finite triangles (+ 0.0; none: +inf, -inf); ha, hb, hc = h - lo; dn = (nx dx + ny dy) + nz dz;
    on_bed  = max(ha, hb, hc) <= bed_tol
    over    = finite & ~on_bed & (dn < -(sin_limit * dbl))         the face looks down more steeply than the limit
    contact = finite &  on_bed & (dn < 0)
and the three terms  over ? dbl : +0.0,  over ? (-dn) * ((ha + hb) + hc) : +0.0,  contact ? dbl : +0.0  (all >= +0.0).  `derive`:
overhang_area = s0 / 2, support_volume = s1 / 6, contact_area = s2 / 2, height = hi - lo.  (h overflowing for coordinates near the
largest float64 is outside the definition.)

support_volume IS A PROXY: the prism from every overhanging face straight down to the bed plane.  It does NOT subtract the part's
own material under an overhang (support that would rest on the part is counted down to the bed), and in a soup of overlapping
solids it counts the faces hidden inside the union like any other.

THE SUM IS A FIXED TREE over the triangle order.  The triangles are cut into chunks of C = 1024 consecutive ones; inside a chunk ONE
accumulator starts at +0.0 and adds the chunk's terms in index order (the last chunk simply ends early).  The chunk partials are
combined exactly like measure_ref.tree_sum combines its partials: groups of 256 padded with +0.0, through `_halve`, repeated until
one value is left.  Every term is >= +0.0, so padding changes no bit."""
import math

import numpy as np

from measure_ref import _halve, cube_soup

C = 1024          # triangles per chunk
LANES = 256
N_SUMS = 3        # sum of dbl over the overhangs; of (-dn) (ha + hb + hc) over them; of dbl over the bed contacts
NEITHER, OVERHANG, CONTACT, NONFINITE = 0, 1, 2, 3
K_BLOCK = 16      # directions taken at once (memory only: the result does not depend on it)


def sin_limit_of(angle):
    """sin of the overhang angle in degrees, 0 <= angle < 90: the steepest overhang from the vertical that prints without support"""
    return math.sin(math.radians(float(angle)))


def normalise(directions):
    """(K, 3) unit directions: d / sqrt((dx*dx + dy*dy) + dz*dz); a zero or non-finite direction is refused"""
    d = np.array(directions, dtype=np.float64)
    if d.ndim == 1:
        d = d.reshape(1, -1)
    if d.ndim != 2 or d.shape[1] != 3 or len(d) < 1:
        raise ValueError('directions must be one vector of 3 components or an array (K, 3) with K >= 1, got shape %r' % (d.shape,))
    if not np.isfinite(d).all():
        raise ValueError('a direction is not finite')
    with np.errstate(all='ignore'):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    if not (np.isfinite(length).all() and (length > 0).all()):
        raise ValueError('a direction is zero (or its length is not a finite float64)')
    return d / length[:, None]


def sphere_directions(n):
    """(n + 6, 3) unit directions: the six axis directions +x, -x, +y, -y, +z, -z, then n points of a Fibonacci spiral"""
    n = int(n)
    if n < 0:
        raise ValueError('sphere_directions: n must be >= 0, got %d' % n)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / max(n, 1)
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = (i + 0.5) * (math.pi * (3.0 - math.sqrt(5.0)))          # (half a turn of the golden angle in: no point on an axis)
    return normalise(np.concatenate([axes, np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)]))


def chunk_tree_sum(terms):
    """the fixed tree over terms (T, ...) float64 in triangle order -> (...): sequential inside a chunk, halving across chunks"""
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    T, rest = terms.shape[0], terms.shape[1:]
    cols = int(np.prod(rest, dtype=np.int64))
    if T == 0:
        return np.zeros(rest)
    n_chunks = -(-T // C)
    padded = np.zeros((n_chunks * C, cols))
    padded[:T] = terms.reshape(T, cols)
    x = padded.reshape(n_chunks, C, cols)
    part = np.zeros((n_chunks, cols))
    for s in range(C):                                  # one accumulator per chunk, in index order
        part = part + x[:, s]
    while True:                                         # (one chunk goes through one group too: x + 0.0 changes no bit of x >= +0.0)
        n_groups = -(-len(part) // LANES)
        padded = np.zeros((n_groups * LANES, cols))
        padded[:len(part)] = part
        part = _halve(padded.reshape(n_groups, LANES, cols))
        if len(part) == 1:
            return part[0].reshape(rest)


def triangle_parts(soup):
    """(tri (T, 3, 3), n (T, 3), dbl (T,), finite (T,)) of a soup"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    finite = np.isfinite(tri).all(axis=(1, 2))
    with np.errstate(all='ignore'):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ux, uy, uz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
        wx, wy, wz = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
        nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
        dbl = np.sqrt((nx * nx + ny * ny) + nz * nz)
    return tri, np.stack([nx, ny, nz], axis=1), dbl, finite


def rate(soup, directions, sin_limit, bed_tol, classes=False):
    """the raw rating of a soup (T, 3, 3) for unit directions (K, 3), used AS GIVEN (what the device receives: `normalise` first):
    dict of lo (K,), hi (K,), sums (K, 3), overhang_triangles (K,), contact_triangles (K,) int64 and, with classes=True,
    classes (K, T) uint8 (0 neither, 1 overhang, 2 contact, 3 non-finite)"""
    tri, n, dbl, finite = triangle_parts(soup)
    D = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    sin_limit, bed_tol = float(sin_limit), float(bed_tol)
    if not (0.0 <= sin_limit < 1.0):
        raise ValueError('sin_limit must lie in [0, 1), got %r' % sin_limit)
    if not (bed_tol >= 0.0):
        raise ValueError('bed_tol must be >= 0, got %r' % bed_tol)
    T, K = len(tri), len(D)
    out = {'lo': np.full(K, np.inf), 'hi': np.full(K, -np.inf), 'sums': np.zeros((K, N_SUMS)),
           'overhang_triangles': np.zeros(K, np.int64), 'contact_triangles': np.zeros(K, np.int64)}
    if classes:
        out['classes'] = np.zeros((K, T), np.uint8)
    if T == 0:
        return out
    with np.errstate(all='ignore'):
        thr = -(sin_limit * dbl)
        for k0 in range(0, K, K_BLOCK):
            d = D[k0:k0 + K_BLOCK]
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]                                  # (k,) against (T, 1)
            h = [(tri[:, v, 0, None] * dx + tri[:, v, 1, None] * dy) + tri[:, v, 2, None] * dz for v in range(3)]      # 3 x (T, k)
            if finite.any():
                hf = np.concatenate([x[finite] for x in h])
                lo, hi = hf.min(axis=0) + 0.0, hf.max(axis=0) + 0.0
            else:
                lo, hi = np.full(len(d), np.inf), np.full(len(d), -np.inf)
            ha, hb, hc = h[0] - lo, h[1] - lo, h[2] - lo
            dn = (n[:, 0, None] * dx + n[:, 1, None] * dy) + n[:, 2, None] * dz
            on_bed = np.maximum(np.maximum(ha, hb), hc) <= bed_tol
            over = finite[:, None] & ~on_bed & (dn < thr[:, None])
            contact = finite[:, None] & on_bed & (dn < 0.0)
            terms = np.stack([np.where(over, dbl[:, None], 0.0), np.where(over, (-dn) * ((ha + hb) + hc), 0.0),
                              np.where(contact, dbl[:, None], 0.0)], axis=2)        # (T, k, 3)
            sl = slice(k0, k0 + len(d))
            out['lo'][sl], out['hi'][sl] = lo, hi
            out['sums'][sl] = chunk_tree_sum(terms)
            out['overhang_triangles'][sl] = over.sum(axis=0)
            out['contact_triangles'][sl] = contact.sum(axis=0)
            if classes:
                cls = np.where(over, OVERHANG, np.where(contact, CONTACT, NEITHER)).astype(np.uint8)
                cls[~finite] = NONFINITE
                out['classes'][sl] = cls.T
    return out


def derive(r):
    """overhang_area, support_volume, contact_area, height (each (K,)) from the raw rating: the factors 1/2 and 1/6 meet the totals
    here, once.  support_volume is the proxy the module's docstring describes."""
    s = np.asarray(r['sums'], dtype=np.float64).reshape(-1, N_SUMS)
    with np.errstate(all='ignore'):
        return {'overhang_area': s[:, 0] / 2.0, 'support_volume': s[:, 1] / 6.0, 'contact_area': s[:, 2] / 2.0,
                'height': np.asarray(r['hi'], dtype=np.float64) - np.asarray(r['lo'], dtype=np.float64)}


def overhangs(soup, directions, angle=45.0, bed_tol=0.0, classes=False):
    """`rate` for directions of any length and an angle in degrees, with the derived values merged in and `directions` (K, 3)"""
    d = normalise(directions)
    r = rate(soup, d, sin_limit_of(angle), bed_tol, classes)
    return dict(r, directions=d, **derive(r))


# ---- the constructed cases the host and the device tests share ----
def box_soup(lo, hi):
    """the 12 outward-facing triangles of the box [lo, hi]: (12, 3, 3)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return (cube_soup(0.0, 1.0) * (hi - lo)) + lo


def t_soup():
    """two boxes forming a T: the stem [0,1] x [0,1] x [0,2] under the bar [-1,2] x [0,1] x [2,3]; the stem's top and the part of the
    bar's underside above it are hidden inside the soup, and are faces like any other: (24, 3, 3)"""
    return np.concatenate([box_soup((0, 0, 0), (1, 1, 2)), box_soup((-1, 0, 2), (2, 1, 3))])
