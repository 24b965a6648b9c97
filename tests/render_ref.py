"""The definition of the sphere-traced render buffers, restated in NumPy over an evaluator
`ev(P) -> values` that the caller passes: the CPU checker (`oracle.evaluate`) or the device interpreter
(`Engine.eval_points`).  The kernel (csrc/sdf_render.hip, k_render) reproduces this bit for bit.

All arithmetic is float64 with one rounding per written operation: a product and a sum are two operations, a quotient is a
division (never a multiplication by a reciprocal), a dot product is (x*x + y*y) + z*z."""
import numpy as np

MISS, HIT, MARCH = 0, 1, 2


def bits(a):
    """the bit patterns of an array (float64 -> int64): what 'bit for bit' compares"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def dot(x, y, z):
    return (x * x + y * y) + z * z


def rays(frame, width, height):
    """origins and unit directions, (height * width, 3) each, row-major; frame = o0, ou, ov, c, du, dv (18 doubles)"""
    o0, ou, ov, c, du, dv = np.asarray(frame, np.float64).reshape(6, 3)
    j, i = np.mgrid[0:height, 0:width]
    i = i.reshape(-1).astype(np.float64)
    j = j.reshape(-1).astype(np.float64)
    O = np.stack([(o0[a] + i * ou[a]) + j * ov[a] for a in range(3)], axis=1)
    d = [(c[a] + i * du[a]) + j * dv[a] for a in range(3)]
    n = np.sqrt(dot(d[0], d[1], d[2]))
    D = np.stack([d[a] / n for a in range(3)], axis=1)
    return O, D


def _at(O, D, t):
    return O + t[:, None] * D


def render(ev, frame, width, height, t_near, t_far, hit_eps, step_scale, normal_eps, max_steps=256, refine=8):
    """dict of depth (h, w) float64, normal (h, w, 3) float64, steps (h, w) int32, status (h, w) uint8"""
    def f(P):
        return np.asarray(ev(np.ascontiguousarray(P)), np.float64).reshape(-1)

    O, D = rays(frame, width, height)
    n = len(O)
    t = np.full(n, float(t_near))
    lo, hi = t.copy(), t.copy()
    status = np.full(n, MARCH, np.int32)
    steps = np.zeros(n, np.int32)
    neg = np.zeros(n, bool)
    step_scale = np.float64(step_scale)
    for _ in range(int(max_steps)):
        m = np.flatnonzero(status == MARCH)
        if not len(m):
            break
        v = f(_at(O[m], D[m], t[m]))
        steps[m] += 1
        nan = v != v
        hit = ~nan & (v < hit_eps)
        go = ~nan & ~hit
        status[m[nan]] = MISS
        status[m[hit]] = HIT
        hi[m[hit]] = t[m[hit]]
        neg[m[hit]] = v[hit] < 0
        g = m[go]
        lo[g] = t[g]
        t[g] = t[g] + v[go] * step_scale
        status[g[t[g] > t_far]] = MISS
    status[status == MARCH] = MISS                       # ran out of steps: steps == max_steps
    r = np.flatnonzero((status == HIT) & neg & (steps > 1))
    for _ in range(int(refine)):
        if not len(r):
            break
        mid = 0.5 * (lo[r] + hi[r])
        v = f(_at(O[r], D[r], mid))
        inside = v < 0
        hi[r[inside]] = mid[inside]
        lo[r[~inside]] = mid[~inside]
    h = np.flatnonzero(status == HIT)
    normal = np.zeros((n, 3))
    if len(h):
        P = _at(O[h], D[h], hi[h])
        g = []
        for a in range(3):
            Pp, Pm = P.copy(), P.copy()
            Pp[:, a] = P[:, a] + normal_eps
            Pm[:, a] = P[:, a] - normal_eps
            g.append(f(Pp) - f(Pm))
        with np.errstate(invalid='ignore', divide='ignore'):
            ln = np.sqrt(dot(g[0], g[1], g[2]))
            N = np.stack([g[a] / ln for a in range(3)], axis=1)
        flat = (ln == 0) | (ln != ln)
        N[flat] = -D[h][flat]
        normal[h] = N
    depth = np.where(status == HIT, hi, np.inf)
    return {'depth': depth.reshape(height, width), 'normal': normal.reshape(height, width, 3),
            'steps': steps.reshape(height, width), 'status': (status == HIT).astype(np.uint8).reshape(height, width)}


def hit_points(buffers, frame):
    """the points O + depth * D of the hits, (n_hits, 3), and their flat pixel indices"""
    h, w = buffers['status'].shape
    O, D = rays(frame, w, h)
    idx = np.flatnonzero(buffers['status'].reshape(-1) == 1)
    return _at(O[idx], D[idx], buffers['depth'].reshape(-1)[idx]), idx


def lockstep_share(steps, tile=(8, 8)):
    """sum(steps) / (64 * sum over tiles of the tile's largest step count): the share of a wave's march evaluations that a
    ray still needed, when a wave takes a tile of `tile` (rows, columns) pixels"""
    h, w = steps.shape
    th, tw = tile
    total = 0
    for y in range(0, h, th):
        for x in range(0, w, tw):
            total += int(steps[y:y + th, x:x + tw].max())
    return float(steps.sum()) / (th * tw * total)
