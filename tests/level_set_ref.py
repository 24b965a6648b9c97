"""NumPy restatement of the device mesh-to-level-set voxelizer (sdf_amd/csrc/sdf_level_set.hip),
in the same float64 operation order, for small meshes (up to a few thousand triangles, work grids up to ~64^3).

It follows the definition, not the kernels: every voxel's squared distance is the minimum over every triangle that can
lie within the background of it (a triangle whose bounding box is farther away is farther away itself, and a distance
at or above the background gives the background either way), and every column is tested against every triangle whose
xy bounding box comes within one voxel of it."""
import numpy as np


def half_width_voxels(voxel_size, half_width=None):
    return 3 if half_width is None else max(3, int(np.ceil(half_width / voxel_size)))


def work_grid(points, vs, hw):
    """first global voxel index and dims of the grid the device computes on"""
    lo = np.floor(points.min(axis=0) / vs) - hw - 1
    hi = np.ceil(points.max(axis=0) / vs) + hw + 1
    return lo.astype(np.int64), (hi - lo + 1).astype(np.int64)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _axpy(a, d, t):
    return (a[0] + d[0] * t, a[1] + d[1] * t, a[2] + d[2] * t)


def _dist2(p, q):
    e = _sub(p, q)
    return _dot(e, e)


def _seg_d2(p, a, b):
    ab = _sub(b, a)
    l = _dot(ab, ab)
    t = _dot(_sub(p, a), ab) / l
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    return np.where(l == 0.0, _dist2(p, a), _dist2(p, _axpy(a, ab, t)))


def tri_d2(p, a, b, c):
    """squared distance of points p (components shaped (m, 1)) to triangles a, b, c (components shaped (1, t)):
    Ericson, Real-Time Collision Detection 5.1.5, the first region that matches wins; a degenerate triangle (zero
    cross product, or a zero denominator in its region) gives the minimum over its three edges"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = _sub(p, b)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = _sub(p, c)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        edges = np.minimum(np.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
        den_ab, den_ac, den_bc = d1 - d3, d2 - d6, e43 + e56
        q_ab = np.where(den_ab == 0.0, edges, _dist2(p, _axpy(a, ab, d1 / den_ab)))
        q_ac = np.where(den_ac == 0.0, edges, _dist2(p, _axpy(a, ac, d2 / den_ac)))
        q_bc = np.where(den_bc == 0.0, edges, _dist2(p, _axpy(b, _sub(c, b), e43 / den_bc)))
        den = va + vb + vc
        inv = 1.0 / den
        v, w = vb * inv, vc * inv
        q_in = np.where(den == 0.0, edges, _dist2(p, _axpy(_axpy(a, ab, v), ac, w)))
        r = np.select([(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
                       (d6 >= 0.0) & (d5 <= d6), (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0)],
                      [_dist2(p, a), _dist2(p, b), q_ab, _dist2(p, c), q_ac, q_bc], default=q_in)
        degen = (ab[1] * ac[2] - ab[2] * ac[1] == 0.0) & (ab[2] * ac[0] - ab[0] * ac[2] == 0.0) & (ab[0] * ac[1] - ab[1] * ac[0] == 0.0)
        return np.where(degen, edges, r)


def _edge(px, py, qx, qy, x, y):
    """resolved sign and value of the projected edge function of P -> Q at (x, y): canonical endpoints (the
    lexicographically smaller is a), E == 0 resolved by the perturbation q + (eps, eps^2)"""
    fwd = (px < qx) | ((px == qx) & (py < qy))
    ax, ay = np.where(fwd, px, qx), np.where(fwd, py, qy)
    bx, by = np.where(fwd, qx, px), np.where(fwd, qy, py)
    dx, dy = bx - ax, by - ay
    e = dx * (y - ay) - dy * (x - ax)
    s = np.sign(e)
    s = np.where(s == 0, np.sign(-dy), s)
    s = np.where(s == 0, np.sign(dx), s)
    return np.where(fwd, s, -s), np.where(fwd, e, -e)


def crossings(x, y, V, vs):
    """the first inside-flip index k0 of every (column, triangle) pair whose triangle covers the column, and the
    column's position in x / y: x, y (m,) column coordinates, V (t, 3, 3) triangle vertices"""
    X, Y = x[:, None], y[:, None]
    v0, v1, v2 = (V[None, :, e] for e in range(3))
    s0, E0 = _edge(v1[..., 0], v1[..., 1], v2[..., 0], v2[..., 1], X, Y)
    s1, E1 = _edge(v2[..., 0], v2[..., 1], v0[..., 0], v0[..., 1], X, Y)
    s2, E2 = _edge(v0[..., 0], v0[..., 1], v1[..., 0], v1[..., 1], X, Y)
    cover = (s0 != 0) & (s0 == s1) & (s0 == s2)
    col, t = np.nonzero(cover)
    E0, E1, E2 = E0[col, t], E1[col, t], E2[col, t]
    z0, z1, z2 = V[t, 0, 2], V[t, 1, 2], V[t, 2, 2]
    s = E0 + E1 + E2
    with np.errstate(divide='ignore', invalid='ignore'):
        zc = np.where(s == 0.0, z0, (E0 * z0 + E1 * z1 + E2 * z2) / s)
    k = np.floor(zc / vs) - 2.0
    for _ in range(5):
        k = np.where(k * vs <= zc, k + 1.0, k)
    return col, k.astype(np.int64)


class _Tris:
    def __init__(self, points, triangles):
        self.V = np.asarray(points, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]     # (t, 3, 3)
        self.lo, self.hi = self.V.min(axis=1), self.V.max(axis=1)

    def near(self, lo, hi, r):
        return np.nonzero(np.all(self.lo <= hi + r, axis=1) & np.all(self.hi >= lo - r, axis=1))[0]


def _min_d2(tr, P, r, chunk=1 << 22):
    """min squared distance of the points P (m, 3) over the triangles within r of their bounding box (inf: none)"""
    cand = tr.near(P.min(axis=0), P.max(axis=0), r)
    out = np.full(len(P), np.inf)
    if len(cand) == 0:
        return out
    V = tr.V[cand]
    a, b, c = ((V[None, :, e, 0], V[None, :, e, 1], V[None, :, e, 2]) for e in range(3))
    step = max(1, chunk // len(cand))
    for s in range(0, len(P), step):
        p = tuple(P[s:s + step, i][:, None] for i in range(3))
        out[s:s + step] = tri_d2(p, a, b, c).min(axis=1)
    return out


def _compose(d2, inside, bg):
    d = np.sqrt(d2)
    v = np.minimum(d, bg).astype(np.float32)
    return np.where(inside & (d != 0.0), -v, v)


def _reach(bg, vs):
    return bg * (1.0 + 1e-6) + vs * 1e-6


def level_set(points, triangles, voxel_size, half_width=None, brick=8):
    """(ijk0, A, background, work grid (lo, dims)) of the device voxelizer, restated"""
    pts = np.asarray(points, dtype=np.float64)
    vs = float(voxel_size)
    hw = half_width_voxels(vs, half_width)
    bg = float(np.float32(hw * vs))
    lo, n = work_grid(pts, vs, hw)
    tr = _Tris(pts, triangles)
    r = _reach(bg, vs)
    d2 = np.full(tuple(n), np.inf)
    for i0 in range(0, n[0], brick):
        for j0 in range(0, n[1], brick):
            for k0 in range(0, n[2], brick):
                I, J, K = np.meshgrid(*(np.arange(s, min(s + brick, m)) for s, m in zip((i0, j0, k0), n)), indexing='ij')
                P = np.stack([(lo[0] + I.ravel()).astype(np.float64) * vs, (lo[1] + J.ravel()).astype(np.float64) * vs,
                              (lo[2] + K.ravel()).astype(np.float64) * vs], axis=1)
                d2[I, J, K] = _min_d2(tr, P, r).reshape(I.shape)
    # parity along +z: flip at k0 (clamped to 0; beyond the grid: nothing), then a running XOR
    I, J = np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing='ij')
    x, y = (lo[0] + I.ravel()).astype(np.float64) * vs, (lo[1] + J.ravel()).astype(np.float64) * vs
    flips = np.zeros((n[0] * n[1], n[2] + 1), dtype=np.int64)
    step = max(1, (1 << 22) // len(tr.V))
    for s in range(0, len(x), step):
        col, k = crossings(x[s:s + step], y[s:s + step], tr.V, vs)
        kw = np.clip(k - lo[2], 0, n[2])
        np.add.at(flips, (col + s, kw), 1)
    inside = (np.cumsum(flips[:, :n[2]], axis=1) & 1).astype(bool).reshape(tuple(n))
    v = _compose(d2, inside, bg)
    act = np.argwhere(np.abs(v) < np.float32(bg))
    a0, a1 = act.min(axis=0), act.max(axis=0)
    A = v[a0[0]:a1[0] + 1, a0[1]:a1[1] + 1, a0[2]:a1[2] + 1]
    return lo + a0, np.ascontiguousarray(A), bg, (lo, n)


def voxel_values(points, triangles, voxel_size, half_width, ijk):
    """the values of the voxels ijk (m, 3) global indices alone (for meshes too large for `level_set`)"""
    pts = np.asarray(points, dtype=np.float64)
    vs = float(voxel_size)
    hw = half_width_voxels(vs, half_width)
    bg = float(np.float32(hw * vs))
    tr = _Tris(pts, triangles)
    r = _reach(bg, vs)
    out = np.empty(len(ijk), dtype=np.float32)
    for q, (i, j, k) in enumerate(np.asarray(ijk, dtype=np.int64)):
        P = np.array([[float(i) * vs, float(j) * vs, float(k) * vs]])
        d2 = _min_d2(tr, P, r)
        cand = np.nonzero((tr.lo[:, 0] <= P[0, 0] + vs) & (tr.hi[:, 0] >= P[0, 0] - vs) &
                          (tr.lo[:, 1] <= P[0, 1] + vs) & (tr.hi[:, 1] >= P[0, 1] - vs))[0]
        _, k0 = crossings(P[:, 0], P[:, 1], tr.V[cand], vs)
        inside = bool(np.count_nonzero(k0 <= k) & 1)
        out[q] = _compose(d2, np.array([inside]), bg)[0]
    return out
