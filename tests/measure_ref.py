"""The definition of a mesh's measurements: the moments of a triangle soup, the values derived from them, and
the edge census of an indexed mesh.  Plain NumPy, float64, one rounding per written operation; no np.dot, `@` or einsum (BLAS
ordering is not ours to pin) and no np.sum over the triangles (its pairwise blocking is not ours either).  csrc/sdf_measure.hip
(k_soup_box, k_soup_moments, k_moment_partials, k_edge_keys, k_edge_classes) reproduces `moments` bit for bit and `edge_census`
exactly; sdf_amd/measure.py restates `derive`.

THE SUM IS A FIXED TREE.  It depends on the order of the triangles and on nothing else.
  * The triangles are cut into chunks of C = 1024 consecutive ones; the last chunk is padded with +0.0 terms.
  * Inside a chunk 256 lanes each start at +0.0 and add their terms in index order: lane l adds the terms of the chunk's triangles
    l, l + 256, l + 512, l + 768.  Then a halving tree combines the lanes: x[:h] + x[h:] for h = 128, 64, ... 1.
  * The chunk partials are cut into groups of 256 consecutive ones, padded with +0.0: one partial per lane, the same halving tree.
    That is repeated on the results until one value is left.  (One chunk: its partial is the total.)
(An accumulator that starts at +0.0 never becomes -0.0, so adding a +0.0 padding term changes no bit.)"""
import numpy as np

C = 1024          # triangles per chunk
LANES = 256
N_SUMS = 11       # |n|; det; det s_x, s_y, s_z; det q_xx, q_yy, q_zz, q_xy, q_xz, q_yz


def _halve(x):
    """x (G, 256, K) -> (G, K): x[:h] + x[h:] for h = 128 ... 1"""
    h = LANES // 2
    while h >= 1:
        x = x[:, :h] + x[:, h:2 * h]
        h //= 2
    return x[:, 0]


def tree_sum(terms):
    """the fixed tree over terms (T, K) float64 in triangle order -> (K,)"""
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    T, K = terms.shape
    if T == 0:
        return np.zeros(K)
    n_chunks = -(-T // C)
    padded = np.zeros((n_chunks * C, K))
    padded[:T] = terms
    x = padded.reshape(n_chunks, C // LANES, LANES, K)
    acc = np.zeros((n_chunks, LANES, K))
    for s in range(C // LANES):                       # each lane adds its triangles in index order
        acc = acc + x[:, s]
    part = _halve(acc)                                # (n_chunks, K)
    while len(part) > 1:
        n_groups = -(-len(part) // LANES)
        padded = np.zeros((n_groups * LANES, K))
        padded[:len(part)] = part
        part = _halve(padded.reshape(n_groups, LANES, K))
    return part[0]


def bounding_box(soup):
    """(finite (T,) bool, lo (3,), hi (3,)) over the triangles whose nine coordinates are all finite; a zero is +0.0; no such
    triangle: lo = +inf, hi = -inf"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    finite = np.isfinite(tri).all(axis=(1, 2))
    P = tri[finite].reshape(-1, 3)
    if len(P) == 0:
        return finite, np.full(3, np.inf), np.full(3, -np.inf)
    lo, hi = P.min(axis=0), P.max(axis=0)
    return finite, lo + 0.0, hi + 0.0                 # (-0.0 + 0.0 = +0.0: the box holds no negative zero)


def triangle_terms(soup, o):
    """(terms (T, 11), zero_area (T,) bool, finite (T,) bool) of a soup (T, 3, 3) about the reference point o"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    o = np.asarray(o, dtype=np.float64)
    finite = np.isfinite(tri).all(axis=(1, 2))
    with np.errstate(all='ignore'):
        a, b, c = tri[:, 0] - o, tri[:, 1] - o, tri[:, 2] - o
        ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
        bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
        cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
        ux, uy, uz = bx - ax, by - ay, bz - az
        wx, wy, wz = cx - ax, cy - ay, cz - az
        nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
        dbl = np.sqrt((nx * nx + ny * ny) + nz * nz)              # the doubled area, the shape of the normals' length
        mx, my, mz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx
        det = (ax * mx + ay * my) + az * mz                       # six times the signed volume
        sx, sy, sz = (ax + bx) + cx, (ay + by) + cy, (az + bz) + cz
        terms = np.stack([
            dbl, det, det * sx, det * sy, det * sz,
            det * (((ax * ax + bx * bx) + cx * cx) + sx * sx),
            det * (((ay * ay + by * by) + cy * cy) + sy * sy),
            det * (((az * az + bz * bz) + cz * cz) + sz * sz),
            det * (((ax * ay + bx * by) + cx * cy) + sx * sy),
            det * (((ax * az + bx * bz) + cx * cz) + sx * sz),
            det * (((ay * az + by * bz) + cy * cz) + sy * sz)], axis=1)
    terms[~finite] = 0.0                                          # a non-finite triangle adds +0.0 to every sum
    return terms, finite & (dbl == 0), finite


def moments(soup, origin=None):
    """the raw totals of a soup (T, 3, 3): dict of sums (11,), origin (3,), box (2, 3), triangles, zero_area, nonfinite.
    origin=None: the midpoint of the bounding box, lo + (hi - lo) / 2, or (0, 0, 0) for an empty box"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    finite, lo, hi = bounding_box(tri)
    if origin is not None:
        o = np.array(origin, dtype=np.float64).reshape(3)
    elif finite.any():
        with np.errstate(all='ignore'):
            o = lo + (hi - lo) / 2.0
    else:
        o = np.zeros(3)
    terms, zero, finite = triangle_terms(tri, o)
    with np.errstate(all='ignore'):
        sums = tree_sum(terms)
    return {'sums': sums, 'origin': o, 'box': np.array([lo, hi]), 'triangles': len(tri), 'zero_area': int(zero.sum()),
            'nonfinite': int((~finite).sum())}


def derive(m):
    """area, volume, centroid (3,), inertia (3, 3) from the totals, in this order of operations.  The factors 1/2, 1/6, 1/24 and
    1/120 meet the totals here, once.  volume <= 0 or a non-finite triangle: centroid and inertia are NaN."""
    s = np.asarray(m['sums'], dtype=np.float64)
    o = np.asarray(m['origin'], dtype=np.float64)
    area = s[0] / 2.0
    volume = s[1] / 6.0
    if not (volume > 0) or m['nonfinite'] > 0:
        return {'area': area, 'volume': volume, 'centroid': np.full(3, np.nan), 'inertia': np.full((3, 3), np.nan)}
    with np.errstate(all='ignore'):
        d = s[2:5] / (4.0 * s[1])                                 # the centroid relative to o: (F / 24) / (D / 6)
        centroid = d + o
        q = s[5:11] / 120.0                                       # second moments about o: xx, yy, zz, xy, xz, yz
        xx, yy, zz = q[0] - volume * d[0] * d[0], q[1] - volume * d[1] * d[1], q[2] - volume * d[2] * d[2]
        xy, xz, yz = q[3] - volume * d[0] * d[1], q[4] - volume * d[0] * d[2], q[5] - volume * d[1] * d[2]
        inertia = np.array([[yy + zz, -xy, -xz],                  # tr(S) I - S at unit density, about the centroid
                            [-xy, xx + zz, -yz],
                            [-xz, -yz, xx + yy]])
    return {'area': area, 'volume': volume, 'centroid': centroid, 'inertia': inertia}


COLLAPSED_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def edge_keys(cells):
    """(keys (3T,) uint64 in cell order, collapsed (T,) bool): min * 2^32 + max * 2 + dir per half-edge (u, v), dir = 1 when
    u > v; the three keys of a collapsed cell are the all-ones sentinel"""
    c = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1, 3)
    collapsed = (c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 2] == c[:, 0])
    u = c.astype(np.uint64)
    v = np.roll(u, -1, axis=1)
    keys = np.minimum(u, v) * np.uint64(1 << 32) + np.maximum(u, v) * np.uint64(2) + (u > v).astype(np.uint64)
    keys[collapsed] = COLLAPSED_KEY
    return keys.reshape(-1), collapsed


def edge_census(cells, n_vertices):
    """the census of an indexed mesh: cells (T, 3) int64, n_vertices.  All integers (closed / oriented: bool)."""
    keys, collapsed = edge_keys(cells)
    k = np.sort(keys[keys != COLLAPSED_KEY])
    und = k >> np.uint64(1)
    start = np.flatnonzero(np.r_[True, und[1:] != und[:-1]]) if len(k) else np.zeros(0, np.int64)
    length = np.diff(np.r_[start, len(k)])
    two = start[length == 2]
    same = ((k[two] ^ k[two + 1]) & np.uint64(1)) == 0
    out = {'vertices': int(n_vertices), 'faces': int(len(collapsed) - collapsed.sum()), 'collapsed': int(collapsed.sum()),
           'paired': int((~same).sum()), 'boundary': int((length == 1).sum()), 'misoriented': int(same.sum()),
           'nonmanifold': int((length >= 3).sum())}
    out['edges'] = out['paired'] + out['boundary'] + out['misoriented'] + out['nonmanifold']
    out['euler'] = out['vertices'] - out['edges'] + out['faces']
    out['closed'] = out['boundary'] == 0 and out['nonmanifold'] == 0
    out['oriented'] = out['misoriented'] == 0
    return out


def measure(points, cells, origin=None):
    """everything of an indexed mesh (points (U, 3), cells (T, 3)): the moments of its soup points[cells], the derived values and
    the census, in one dict"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    m = moments(points[cells], origin)
    out = dict(derive(m), bounds=m['box'], triangles=m['triangles'], zero_area_triangles=m['zero_area'],
               nonfinite_triangles=m['nonfinite'], origin=m['origin'], sums=m['sums'])
    out.update(edge_census(cells, len(points)))
    return out


# ---- the constructed cases the host and the device tests share ----
def cube_soup(lo=0.5, hi=1.5, shift=(0.0, 0.0, 0.0)):
    """the 12 outward-facing triangles of the cube [lo, hi]^3, translated by `shift`: (12, 3, 3)"""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float64)      # index = 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]       # -x, +x, -y, +y, -z, +z
    tris = []
    for p, q, r, s in quads:
        tris += [(p, q, r), (p, r, s)]
    return v[np.array(tris)] + np.asarray(shift, dtype=np.float64)


def tetrahedron_soup():
    """the right tetrahedron with unit legs at the origin, outward: (4, 3, 3)"""
    o, x, y, z = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    return np.array([[o, y, x], [o, x, z], [o, z, y], [x, y, z]])


def weld(soup):
    """(points, cells) of a soup, as np.unique welds it"""
    pts, inv = np.unique(np.asarray(soup, dtype=np.float64).reshape(-1, 3), axis=0, return_inverse=True)
    return pts, np.asarray(inv).reshape(-1, 3).astype(np.int64)


def census_cases():
    """name -> (soup (T, 3, 3), expected counts): the constructed cases of the census"""
    cube = cube_soup()
    flipped = cube.copy()
    flipped[5] = flipped[5][[0, 2, 1]]
    # ('open': the missing face takes its diagonal with it, 18 - 1 edges)  a second cube that shares exactly the edge x = 1.5, y = 1.5 with the first
    twin = cube_soup(shift=(1.0, 1.0, 0.0))
    collapsed = np.concatenate([cube, [[cube[0, 0], cube[0, 0], cube[0, 1]]]])
    return {
        'cube': (cube, dict(vertices=8, edges=18, faces=12, euler=2, paired=18, boundary=0, misoriented=0, nonmanifold=0,
                            collapsed=0, closed=True, oriented=True)),
        'open': (cube[2:], dict(vertices=8, edges=17, faces=10, paired=13, boundary=4, nonmanifold=0, misoriented=0,
                                closed=False, oriented=True)),
        'flipped': (flipped, dict(vertices=8, edges=18, faces=12, paired=15, misoriented=3, boundary=0, nonmanifold=0,
                                  closed=True, oriented=False)),
        'twins': (np.concatenate([cube, twin]), dict(vertices=14, edges=35, faces=24, paired=34, nonmanifold=1, boundary=0,
                                                     misoriented=0, closed=False, oriented=True)),
        'collapsed': (collapsed, dict(vertices=8, edges=18, faces=12, collapsed=1, paired=18, euler=2, closed=True, oriented=True)),
        'empty': (np.zeros((0, 3, 3)), dict(vertices=0, edges=0, faces=0, collapsed=0, euler=0, closed=True, oriented=True)),
    }


def book_soup(k, n_pad):
    """n_pad unrelated triangles, then a book of k triangles around one edge.  Every padding vertex sorts before the book's, and the
    edge's two vertices before the pages' tips: in the sorted keys the edge's run is [3 n_pad, 3 n_pad + k)"""
    rng = np.random.RandomState(100 * k + n_pad)
    pad = rng.uniform(-3.0, -2.0, size=(n_pad, 3, 3))
    u, v = np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    pages = []
    for j in range(k):
        ang = 2 * np.pi * j / 5
        pages.append([u, v, np.array([1.0 + np.cos(ang), np.sin(ang) + 2.0, 0.5])])
    return np.concatenate([pad, np.array(pages).reshape(k, 3, 3)])
