"""Ground truth for the mesh-to-level-set voxelizer, written from the geometry and not from the algorithm under test
(csrc/sdf_level_set.hip and its restatement tests/level_set_ref.py): the true distance of a point to a triangle is the
distance to its plane where the projection falls inside it and the distance to its nearest side otherwise, and a point is
inside a closed mesh where the mesh's generalised winding number is not zero.  No region cascade, no edge functions, no
column parity.  NumPy only; neither the package nor the restatement is imported.

Also here: the rules a voxel grid is held to against that truth (`hold`), and the catalogue of small meshes that the host
and the device tests share (`CASES`, `OPEN_PREFIXES`), with the mesh builders they use."""
import collections
import concurrent.futures
import functools
import os

import numpy as np

# Distances are computed in the widest float NumPy has.  On x86-64 that is the 80-bit extended format (eps 1.1e-19), and
# that is what ran when the figures in the tests' docstrings were taken; where long double is no wider than float64
# (eps 2.2e-16), float64 runs: its error of ~1e-15 on these meshes is still eight orders below the float32 ulp of the bound.
WIDE = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64

# A voxel within ON_SURFACE of the mesh is "on the surface": its sign is not asked, and its magnitude must be the distance to
# ZERO.  (For a voxel exactly on the mesh that is |v| < 1e-12, the rule of the host test of ties.  Stated as "|v| < 1e-12" for
# the whole class the rule was wrong: the example model's flat faces lie 5.6e-10 from a voxel plane, and 5.6e-10 is what those
# voxels must hold.)
ON_SURFACE = 1e-9
ZERO = 1e-12


def half_width_voxels(voxel_size, half_width=None):
    return 3 if half_width is None else max(3, int(np.ceil(half_width / voxel_size)))


def _rows(X):
    return X[:, 0][None, :], X[:, 1][None, :], X[:, 2][None, :]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _side_d2(r, d, l):
    """squared distance to the segment p0 + [0, 1] d of the points at r = q - p0: the parameter of the foot, clamped"""
    t = np.clip((r[0] * d[0] + r[1] * d[1] + r[2] * d[2]) / l, 0, 1)
    ex, ey, ez = r[0] - t * d[0], r[1] - t * d[1], r[2] - t * d[2]
    return ex * ex + ey * ey + ez * ez


def _boxes(V):
    """the bounding boxes of the triangles, (3, t) each: low corners, high corners"""
    return np.ascontiguousarray(V.min(axis=1).T), np.ascontiguousarray(V.max(axis=1).T)


def true_d2(Q, V, reach=None, boxes=None, chunk=1 << 16):
    """minimum squared distance of the points Q (m, 3) to the triangles V (t, 3, 3), in WIDE.  With `reach`, only the
    triangles whose bounding box comes within `reach` of the points' bounding box are looked at (inf where there is none):
    exact for every point whose distance is below `reach`.  `boxes`: `_boxes(V)`, where the caller has them."""
    Q, V = np.asarray(Q, dtype=np.float64), np.asarray(V, dtype=np.float64)
    out = np.full(len(Q), np.inf, dtype=WIDE)
    if reach is not None and len(Q):
        lo, hi = boxes if boxes is not None else _boxes(V)
        V = V[np.all(lo <= (Q.max(axis=0) + reach)[:, None], axis=0) & np.all(hi >= (Q.min(axis=0) - reach)[:, None], axis=0)]
    if len(V) == 0 or len(Q) == 0:
        return out
    Q, V = Q.astype(WIDE), V.astype(WIDE)
    a, b, c = V[:, 0], V[:, 1], V[:, 2]
    n = _cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    # ((b - a) x (q - a)) . n = (q - a) . (n x (b - a)): the inward normal of each side within the plane, per triangle
    inward = [_rows(_cross(n, e)) for e in (b - a, c - b, a - c)]
    corner = [_rows(p) for p in (a, b, c)]
    side = [_rows(e) for e in (b - a, c - b, a - c)]
    length = [np.where(l == 0, 1, l)[None, :] for l in ((e * e).sum(axis=1) for e in (b - a, c - b, a - c))]   # (a point: d = 0, any t)
    nx, ny, nz = _rows(n)
    flat, nn1 = (nn > 0)[None, :], np.where(nn > 0, nn, 1)[None, :]
    step = max(1, chunk // len(V))
    for s in range(0, len(Q), step):
        q = [Q[s:s + step, i][:, None] for i in range(3)]
        r = [[q[i] - p[i] for i in range(3)] for p in corner]
        within = flat
        for rr, m in zip(r, inward):
            within = within & (rr[0] * m[0] + rr[1] * m[1] + rr[2] * m[2] >= 0)
        h = r[0][0] * nx + r[0][1] * ny + r[0][2] * nz
        sides = np.minimum(np.minimum(_side_d2(r[0], side[0], length[0]), _side_d2(r[1], side[1], length[1])), _side_d2(r[2], side[2], length[2]))
        out[s:s + step] = np.where(within, h * h / nn1, sides).min(axis=1)
    return out


def winding(Q, V, chunk=1 << 17):
    """generalised winding number of the triangles V (t, 3, 3) about the points Q (m, 3): the sum of their signed solid
    angles over 4 pi (van Oosterom and Strackee), float64"""
    Q, V = np.asarray(Q, dtype=np.float64), np.asarray(V, dtype=np.float64)
    out = np.zeros(len(Q))
    if len(V) == 0:
        return out
    # tiles of `chunk` (point, triangle) pairs: temporaries of 1 MB, large enough that threads spend their time in NumPy's
    # loops; a point's tiles are summed in the order of the triangles whatever the number of threads
    cols = min(len(V), chunk)
    rows = max(1, chunk // cols)
    corner = [[np.ascontiguousarray(V[:, e, i]) for i in range(3)] for e in range(3)]

    def block(s):
        q = [Q[s:s + rows, i][:, None] for i in range(3)]
        acc = np.zeros(len(q[0]))
        for c in range(0, len(V), cols):
            (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ([p[i][None, c:c + cols] - q[i] for i in range(3)] for p in corner)
            la, lb, lc = np.sqrt(ax * ax + ay * ay + az * az), np.sqrt(bx * bx + by * by + bz * bz), np.sqrt(cx * cx + cy * cy + cz * cz)
            det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
            den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb
            acc += np.arctan2(det, den).sum(axis=1)
        out[s:s + rows] = acc

    starts = range(0, len(Q), rows)
    if len(Q) * len(V) < 1 << 24:
        for s in starts:
            block(s)
    else:                                                 # (NumPy's loops release the interpreter lock)
        with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
            list(pool.map(block, starts))
    return out / (2 * np.pi)


Truth = collections.namedtuple('Truth', 'want inside on_surface d w bg ijk0')


def voxel_points(ijk0, shape, vs):
    """the float64 positions (index times voxel size) of the voxels of an index box, (m, 3), k fastest"""
    I, J, K = np.meshgrid(*(np.arange(n, dtype=np.int64) + int(o) for n, o in zip(shape, ijk0)), indexing='ij')
    return np.stack([I.ravel().astype(np.float64) * vs, J.ravel().astype(np.float64) * vs, K.ravel().astype(np.float64) * vs], axis=1)


def expected(P, T, vs, half_width, ijk0, shape, closed=True, brick=8):
    """the truth on the index box ijk0 + [0, shape): `want` = min(d, background) in float64, `inside` (the winding number
    rounds to something other than 0; None for an open mesh), `on_surface` = d <= 1e-9; and with them the distance d
    unclamped (inf: farther than the background), the winding number w and the background"""
    P = np.asarray(P, dtype=np.float64)
    vs = float(vs)
    V = P[np.asarray(T, dtype=np.int64)]
    bg = float(np.float32(half_width_voxels(vs, half_width) * vs))
    shape = tuple(int(n) for n in shape)
    d = np.full(shape, np.inf)
    reach = bg * (1 + 1e-6) + vs * 1e-6
    boxes = _boxes(V)
    for i in range(0, shape[0], brick):
        for j in range(0, shape[1], brick):
            for k in range(0, shape[2], brick):
                sub = tuple(min(brick, n - o) for n, o in zip(shape, (i, j, k)))
                Q = voxel_points((ijk0[0] + i, ijk0[1] + j, ijk0[2] + k), sub, vs)
                d[i:i + sub[0], j:j + sub[1], k:k + sub[2]] = np.sqrt(true_d2(Q, V, reach, boxes)).astype(np.float64).reshape(sub)
    w = winding(voxel_points(ijk0, shape, vs), V).reshape(shape) if closed else None
    inside = np.rint(w) != 0 if closed else None
    return Truth(np.minimum(d, bg), inside, d <= ON_SURFACE, d, w, bg, np.asarray(ijk0, dtype=np.int64))


def expected_at(P, T, vs, half_width, ijk):
    """the truth of the voxels ijk (m, 3) alone, each with its own candidates: for meshes too large for a dense grid"""
    P = np.asarray(P, dtype=np.float64)
    vs = float(vs)
    V = P[np.asarray(T, dtype=np.int64)]
    bg = float(np.float32(half_width_voxels(vs, half_width) * vs))
    Q = np.asarray(ijk, dtype=np.int64).astype(np.float64) * vs
    reach = bg * (1 + 1e-6) + vs * 1e-6
    boxes = _boxes(V)
    d = np.array([float(np.sqrt(true_d2(q[None, :], V, reach, boxes)[0])) for q in Q])
    w = winding(Q, V)
    return Truth(np.minimum(d, bg), np.rint(w) != 0, d <= ON_SURFACE, d, w, bg, None)


def truth_grid(P, T, vs, half_width=None, closed=True):
    """the truth on a grid that holds every voxel nearer than the background, and a ring of farther ones around them: a voxel
    within hw voxel sizes of the mesh lies within hw voxels of the index box of its points"""
    P = np.asarray(P, dtype=np.float64)
    hw = half_width_voxels(vs, half_width)
    lo = np.floor(P.min(axis=0) / vs).astype(np.int64) - hw - 1
    hi = np.ceil(P.max(axis=0) / vs).astype(np.int64) + hw + 1
    return expected(P, T, vs, half_width, lo, hi - lo + 1, closed)


def _index_box(m):
    i = np.argwhere(m)
    return i.min(axis=0), i.max(axis=0)


def hold(ijk0, A, truth, sign='winding', near_background=0):
    """Holds the cropped grid (ijk0, A) of the code under test to `truth` (of `truth_grid`) and returns the figures.
      magnitude   off the surface | |v| - want | <= one float32 ulp of the background: the float64 error of either
                  formulation is ~1e-15, so v is the correctly rounded float32(want) or its neighbour;
      sign        off the surface (v < 0) == inside, no exceptions, where inside is round(w) != 0 (`sign='parity'`:
                  round(w) odd, for a mesh listed twice; `sign=None`: an open mesh, no truth); w is an integer to 1e-6 there;
      surface     where d <= 1e-9 only | |v| - d | < 1e-12 (for d = 0: |v| < 1e-12), whatever the sign;
      box         (ijk0, A.shape) is the index box of float32(want) < float32(background); voxels whose distance is within
                  one float32 ulp of the background may fall either way: there must be exactly `near_background` of them."""
    A = np.asarray(A)
    assert A.dtype == np.float32
    bg32 = np.float32(truth.bg)
    ulp = float(np.spacing(bg32))
    o = np.asarray(ijk0, dtype=np.int64) - truth.ijk0
    assert np.all(o >= 0) and np.all(o + A.shape <= truth.want.shape), (ijk0, A.shape, truth.ijk0, truth.want.shape)
    active = truth.want.astype(np.float32) < bg32
    near = np.abs(truth.d - truth.bg) <= ulp
    assert np.count_nonzero(near) == near_background, np.count_nonzero(near)
    (s0, s1), (m0, m1) = _index_box(active & ~near), _index_box(active | near)
    assert np.all(m0 <= o) and np.all(o <= s0) and np.all(s1 <= o + A.shape - 1) and np.all(o + A.shape - 1 <= m1), (o, A.shape, s0, s1, m0, m1)
    box = tuple(slice(o[a], o[a] + A.shape[a]) for a in range(3))
    want, on, d, v = truth.want[box], truth.on_surface[box], truth.d[box], A.astype(np.float64)
    off = ~on
    err = np.abs(np.abs(v) - want)
    assert np.all(err[off] <= ulp), (err[off].max() / ulp, np.count_nonzero(err[off] > ulp))
    assert np.all(np.abs(np.abs(v[on]) - d[on]) < ZERO), np.abs(np.abs(v[on]) - d[on]).max()
    if sign is not None:
        w = truth.w[box]
        assert np.all(np.abs(w - np.rint(w))[off] < 1e-6), np.abs(w - np.rint(w))[off].max()
        inside = (np.rint(w).astype(np.int64) & 1) != 0 if sign == 'parity' else truth.inside[box]
        assert np.array_equal(v[off] < 0, inside[off]), np.count_nonzero(((v < 0) != inside) & off)
    return {'shape': A.shape, 'voxels': A.size, 'on_surface': int(np.count_nonzero(on)), 'max_ulp': float(err[off].max() / ulp),
            'near_background': int(np.count_nonzero(near)), 'negative': int(np.count_nonzero(v < 0))}


# ---- meshes

# the 12 triangles of the unit cube [0, 1]^3, outward
CUBE_P = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
CUBE_T = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                   [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return lo + CUBE_P * (hi - lo), CUBE_T.copy()


def torus_mesh(R=0.6, r=0.25, nu=32, nv=16):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    P = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    T = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return P, T


def icosphere(level=3, radius=1.0):
    t = (1 + 5 ** 0.5) / 2
    P = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    P = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in P]
    T = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = P[a] + P[b]
                P.append(q / np.linalg.norm(q))
                mid[k] = len(P) - 1
            return mid[k]
        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        T = nt
    return np.array(P) * radius, np.array(T)


def octahedron(r=0.5):
    """vertices at +-r on the axes (+x, -x, +y, -y, +z, -z), 8 faces, outward"""
    P = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], dtype=np.float64)
    T = [[x, y, z] if (x + y + z) % 2 == 0 else [y, x, z] for x in (0, 1) for y in (2, 3) for z in (4, 5)]
    return P, np.array(T)


def tetrahedron(a, b, c, d):
    """outward: every face turns its normal away from the fourth vertex"""
    P = np.array([a, b, c, d], dtype=np.float64)
    T = []
    for f, o in ([0, 1, 2], 3), ([0, 1, 3], 2), ([0, 2, 3], 1), ([1, 2, 3], 0):
        n = np.cross(P[f[1]] - P[f[0]], P[f[2]] - P[f[0]])
        T.append(f if n @ (P[o] - P[f[0]]) < 0 else [f[1], f[0], f[2]])
    return P, np.array(T)


def rot(seed):
    """a rotation in general position: the Q of a seeded normal matrix, made proper"""
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))[0]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


Case = collections.namedtuple('Case', 'points triangles voxel_size half_width ties sign near_background')


def _case(mesh, vs, half_width=None, turn=None, shift=None, ties=False, sign='winding', near_background=0):
    P, T = mesh
    if turn is not None:
        P = P @ rot(turn).T
    if shift is not None:
        P = P + np.asarray(shift, dtype=np.float64)
    return Case(P, T, vs, half_width, ties, sign, near_background)


def _catalogue():
    """The smallest meshes that still reach the path named (grids under about 32^3 but the tall one, at most 500 triangles).
    `ties`: many voxels lie on the surface (more than 50 are asked for); otherwise at most 2 may.
    `near_background`: how many voxels of the truth's grid have a distance within one float32 ulp of the background, counted
    on the CPU from the truth alone.  Every one of them is a tie d = hw * vs of the geometry, explained at its case; the
    background float32(hw * vs) lies 0 to 0.4 ulp above that and the rounding boundary half an ulp below it, so such a voxel
    rounds to the background whichever way the last bits of d fall."""
    octa = octahedron(0.5)
    wide = (octa[0] * (1.0, 0.5, 1.5), octa[1])
    box = box_mesh((-0.43, -0.31, -0.27), (0.52, 0.36, 0.33))
    # the dyadic octahedron on a dyadic grid: a voxel 3 steps along an axis from a vertex, or (2, 2, 1) steps (4 + 4 + 1 = 9),
    # is exactly the background away from it
    near_octa = 126
    return {
        # every vertex and the whole z = 0 rim on voxel centres; the column at (0, 0) runs through the two apexes, where four
        # sloping faces meet; the projected edges x +- y = +-0.5 run through column centres
        'octa_ties': _case(octa, 0.125, ties=True, near_background=near_octa),
        # the same far away: a large and a negative g.lo, ties kept exactly (dyadic offsets)
        'octa_ties_far': _case(octa, 0.125, shift=np.array([-40, 24, 800]) * 0.125, ties=True, near_background=near_octa),
        # a band of 6 voxels, two mask words (dyadic as well: 6 steps along an axis from a vertex, (4, 4, 2) steps)
        'octa_wide_band': _case(wide, 0.0625, 0.35, ties=True, near_background=78),
        # faces and edges in general position (the origin is a voxel and lies 0.27 = 3 * 0.09 inside the face z = -0.27, turned or not)
        'box_rot': _case(box, 0.09, turn=1, near_background=1),
        # and far from the origin, mixed signs
        'box_rot_far': _case(box, 0.09, turn=2, shift=(100.3, -57.1, 31.7)),
        # a wall six times thinner than a voxel, sliver triangles (aspect 200), two crossings inside one voxel step
        'thin_plate': _case(box_mesh((-1.0, -0.005, -0.15), (1.0, 0.005, 0.15)), 0.06, turn=3),
        # 480 triangles, columns through the tilted hole
        'torus_rot': _case(torus_mesh(0.6, 0.25, 24, 10), 0.07, turn=4),
        # obtuse faces, where the order of the vertex and edge regions decides (the vertex at the origin stays there: 13 of the
        # 30 voxels 3 or (2, 2, 1) steps from it have it as their nearest point)
        'obtuse_tet': _case(tetrahedron((0, 0, 0), (1, 0, 0), (0.5, 0.05, 0), (0.5, 0.02, 0.6)), 0.05, turn=5, near_background=13),
        # a work grid of 65 or more voxels along z: three mask words, every voxel checked (the columns 0.09 and 0.12 beside
        # the vertical edges x = -0.21, y = 0.18 and x = 0.23, y = -0.19 are 0.15 = 3 * 0.05 from them: 3-4-5)
        'tall': _case(box_mesh((-0.21, -0.19, -1.63), (0.23, 0.18, 1.71)), 0.05, near_background=90),
        # 320 triangles inside one voxel's neighbourhood: every wave contends for the same few words
        'crumb': _case(icosphere(2, radius=0.02), 0.05, shift=(0.013, -0.007, 0.021)),
        # every triangle twice: the crossings cancel in pairs, no voxel is negative, the winding number inside is 2
        'doubled': _case((octa[0], np.vstack([octa[1], octa[1]])), 0.125, ties=True, sign='parity', near_background=near_octa),
    }


CASES = _catalogue()
# the first 1, 2, 3 and 5 triangles of `octa_ties`, and their voxels exactly the background away (as there)
OPEN_PREFIXES = {1: 66, 2: 88, 3: 107, 5: 124}


def open_prefix(nt):
    """the first nt triangles of `octa_ties`, all six points kept: an open mesh, which has no winding-number truth"""
    c = CASES['octa_ties']
    return Case(c.points, c.triangles[:nt], c.voxel_size, c.half_width, None, None, OPEN_PREFIXES[nt])


def get_case(name):
    return open_prefix(int(name[4:])) if name.startswith('open') else CASES[name]


NAMES = tuple(CASES) + tuple('open%d' % n for n in OPEN_PREFIXES)


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """the truth of a catalogue case (or of 'open<nt>'), computed once for all the tests of a run; read only"""
    c = get_case(name)
    t = truth_grid(c.points, c.triangles, c.voxel_size, c.half_width, closed=c.sign is not None)
    for x in t:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return t


def hold_case(name, ijk0, A, work=None):
    """a catalogue case's grid against its truth (`hold`), the share of its voxels on the surface, and, given the work grid
    (lo, dims) the grid was computed on, that the case still reaches the path it is there for; returns the figures"""
    c = get_case(name)
    f = hold(ijk0, A, case_truth(name), c.sign, c.near_background)
    if c.ties is not None:
        # in general position at most 2 voxels on the surface (a grid point can fall within 1e-9 of a turned face by chance);
        # a tie case more than 50, or it is not testing ties; no case more than 5 % of its voxels
        n = f['on_surface']
        assert (n > 50) if c.ties else (n <= 2), n
        assert n <= 0.05 * f['voxels'], (n, f['voxels'])
    if name == 'doubled':
        assert f['negative'] == 0
    elif c.sign is not None and name != 'crumb':          # (the crumb holds no voxel)
        assert f['negative'] > 0
    if work is not None:
        lo, n = work
        words = {'tall': 3, 'octa_wide_band': 2, 'thin_plate': 2}.get(name, 1)
        assert (int(n[2]) + 31) // 32 == words, n
        if name == 'octa_ties_far':
            assert lo[0] < -40 and lo[1] > 0 and lo[2] > 780
        if name == 'box_rot_far':
            assert lo[0] > 1000 and lo[1] < -600 and lo[2] > 300
    f['work'] = None if work is None else tuple(int(x) for x in work[1])
    return f
