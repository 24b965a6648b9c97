"""The definition of the wall-thickness probe, in NumPy over an evaluator `ev(P) -> (N,) float64` that the
caller passes: the CPU checker (`oracle.evaluate`) or the device interpreter (`Engine.eval_points`).  csrc/sdf_thickness.hip
(k_vertex_thickness) reproduces it bit for bit, sdf_amd/thickness.py (`vertex_thickness`) restates it for the host path.

From every vertex a ray is sphere-traced INWARD -- along the negated field normal -- through the solid until the field turns
positive again; the bracket of that crossing is bisected; the ray's length is the wall's ray thickness at the vertex.

All arithmetic is float64 with one rounding per written operation: a product and a sum are two operations, a quotient is a
division (never a multiplication by a reciprocal), a dot product is (x*x + y*y) + z*z, a point on a ray is p + t * d."""
import numpy as np

OPEN, THICK, THIN, FLAT, NAN = 0, 1, 2, 3, 4
_MARCH = 5                                   # (inside the march only)
NAMES = ('OPEN', 'THICK', 'THIN', 'FLAT', 'NAN')


def bits(a):
    """the bit patterns of an array (float64 -> int64): what 'bit for bit' compares"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def directions(ev, P, normal_eps):
    """(D (U, 3), flat (U,) bool): the inward ray directions -(g / len) of the definition of normals_ref.py -- for axis k the value
    at x_k + eps minus the value at x_k + (-eps), len = sqrt((g0*g0 + g1*g1) + g2*g2) -- and which vertices have none (len 0 or NaN)"""
    eps = np.float64(normal_eps)
    U = len(P)
    g = np.zeros((U, 3), np.float64)
    for k in range(3):
        plus = P.copy()
        plus[:, k] = P[:, k] + eps
        minus = P.copy()
        minus[:, k] = P[:, k] + (-eps)
        v_plus = np.asarray(ev(plus), dtype=np.float64).reshape(-1) if U else np.zeros(0)
        v_minus = np.asarray(ev(minus), dtype=np.float64).reshape(-1) if U else np.zeros(0)
        g[:, k] = v_plus - v_minus
    g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ln = np.sqrt((g0 * g0 + g1 * g1) + g2 * g2)
        flat = (ln == 0) | (ln != ln)
        D = -(g / ln[:, None])
    D[flat] = 0.0
    return D, flat


def thickness(ev, P, normal_eps, start, min_step, t_far, step_scale=1.0, max_steps=256, refine=16, debug=False):
    """(thickness (U,) float64, status (U,) uint8, steps (U,) int32) at the points P (U, 3); with debug=True a fourth value: a dict
    of `D` (the ray directions), `lo`, `hi` (the bracket the definition ends with) and `bracket` (hi - lo at the end of the march)"""
    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), np.float64).reshape(-1)

    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    U = len(P)
    start, min_step, t_far, step_scale = np.float64(start), np.float64(min_step), np.float64(t_far), np.float64(step_scale)
    D, flat = directions(ev, P, normal_eps)
    t = np.full(U, start)
    lo = np.zeros(U)
    hi = np.full(U, start)
    status = np.where(flat, FLAT, _MARCH).astype(np.int32)
    steps = np.zeros(U, np.int32)
    for k in range(int(max_steps)):
        m = np.flatnonzero(status == _MARCH)
        if not len(m):
            break
        v = f(P[m] + t[m][:, None] * D[m])
        steps[m] += 1
        nan = v != v
        out = ~nan & (v >= 0)
        go = ~nan & ~out
        status[m[nan]] = NAN
        status[m[out]] = THIN if k == 0 else THICK       # the first pass: nothing solid lies `start` inside the vertex
        hi[m[out]] = t[m[out]]
        g = m[go]
        lo[g] = t[g]
        adv = (-v[go]) * step_scale
        t[g] = t[g] + np.where(adv > min_step, adv, min_step)
        status[g[t[g] > t_far]] = OPEN
    status[status == _MARCH] = OPEN                      # ran out of steps: steps == max_steps
    bracket = hi - lo
    r = np.flatnonzero(status == THICK)
    for _ in range(int(refine)):
        if not len(r):
            break
        mid = 0.5 * (lo[r] + hi[r])
        inside = f(P[r] + mid[:, None] * D[r]) < 0
        lo[r[inside]] = mid[inside]
        hi[r[~inside]] = mid[~inside]                    # (NaN included)
    th = np.full(U, np.nan)
    solid = (status == THICK) | (status == THIN)
    th[solid] = hi[solid]
    th[status == OPEN] = np.inf
    out = (th, status.astype(np.uint8), steps)
    return out + ({'D': D, 'lo': lo, 'hi': hi, 'bracket': bracket},) if debug else out


def ply_header(U, T, with_normals, quality=False):
    lines = ['ply', 'format binary_little_endian 1.0', 'comment sdf_amd', 'element vertex %d' % U, 'property float x', 'property float y',
             'property float z']
    if with_normals:
        lines += ['property float nx', 'property float ny', 'property float nz']
    if quality:
        lines += ['property float quality']
    lines += ['element face %d' % T, 'property list uchar int vertex_indices', 'end_header']
    return ''.join(l + '\n' for l in lines).encode('ascii')


def parse_ply(path):
    """(points float32 (U, 3), normals float32 (U, 3) or None, quality float32 (U,) or None, cells int32 (T, 3), header bytes) of a
    file this project writes"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    head = raw[:end].decode('ascii').split('\n')
    U = int([l for l in head if l.startswith('element vertex')][0].split()[-1])
    T = int([l for l in head if l.startswith('element face')][0].split()[-1])
    wn, wq = 'property float nx' in head, 'property float quality' in head
    w = 3 + (3 if wn else 0) + (1 if wq else 0)
    assert len(raw) == end + U * 4 * w + T * 13, (len(raw), end, U, T, w)
    v = np.frombuffer(raw, '<f4', U * w, end).reshape(U, w)
    f = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), T, end + U * 4 * w)
    assert (f['n'] == 3).all()
    return v[:, :3], (v[:, 3:6] if wn else None), (v[:, w - 1] if wq else None), f['v'], raw[:end]


def lockstep_share(steps, wave=64):
    """sum(steps) / (wave * sum over runs of `wave` vertices, in weld order, of the run's largest step count): the share of a wave's
    march evaluations that a vertex still needed"""
    steps = np.asarray(steps)
    total = sum(int(steps[i:i + wave].max()) for i in range(0, len(steps), wave))
    return float(steps.sum()) / (wave * total) if total else 1.0
