"""The definition of a mesh held to the field, in NumPy over an evaluator `ev(P) -> (N,) float64` that the
caller passes: the CPU checker (`oracle.evaluate`) or the device interpreter (`Engine.eval_points`).  csrc/sdf_deviation.hip
(k_triangle_deviation, k_vertex_snap) reproduces it bit for bit, sdf_amd/deviation.py restates it for the host path.

`deviation`: how far every triangle of a soup lies from the zero set, sampled on a barycentric lattice.  `snap`: the welded vertices
put back on the zero set by Newton steps along the central-difference gradient.

All arithmetic is float64 with one rounding per written operation: a product and a sum are two operations, a quotient is a
division (never a multiplication by a reciprocal), a dot product is (x*x + y*y) + z*z, a sample point is (A*wa + B*wb) + C*wc, a
Newton step is q - s * g."""
import numpy as np

LEFT, SNAPPED, HELD, FLAT, NAN = 0, 1, 2, 3, 4
_ITER = 5                                    # (inside the passes only)
NAMES = ('LEFT', 'SNAPPED', 'HELD', 'FLAT', 'NAN')


def bits(a):
    """the bit patterns of an array (float64 -> int64): what 'bit for bit' compares"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    """elementwise: the same bits, or a NaN on both sides (IEEE 754 does not fix a NaN's sign and payload, and the checker's libm-free
    C and the device differ in them)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float64:
        return a == b
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def n_samples(order):
    return (order + 1) * (order + 2) // 2


def weights(order):
    """(S, 3) float64: wa, wb, wc of the S samples, in the order for i in 0..n: for j in 0..n-i"""
    n = int(order)
    if not 1 <= n <= 8:
        raise ValueError('order must lie in 1 .. 8, got %r' % (order,))
    dn = np.float64(n)
    return np.array([[np.float64(n - i - j) / dn, np.float64(i) / dn, np.float64(j) / dn] for i in range(n + 1) for j in range(n + 1 - i)],
                    np.float64).reshape(-1, 3)


def sample_points(soup, order):
    """(T, S, 3) float64: (A*wa + B*wb) + C*wc per coordinate"""
    tri = np.ascontiguousarray(soup, dtype=np.float64).reshape(-1, 3, 3)
    W = weights(order)
    A, B, C = tri[:, None, 0, :], tri[:, None, 1, :], tri[:, None, 2, :]
    return (A * W[None, :, 0, None] + B * W[None, :, 1, None]) + C * W[None, :, 2, None]


def deviation(ev, soup, order):
    """(dev (T,) float64, at (T,) int32, sumsq (T,) float64) of the soup (T, 3, 3): the sampled value of largest magnitude -- a later
    sample replaces it only where |v| is strictly greater, the first NaN sample replaces it for good --, the index of that sample,
    and the sequential sum of v*v in sample order"""
    Q = sample_points(soup, order)
    T, S = Q.shape[:2]
    dev, at, sumsq = np.zeros(T), np.zeros(T, np.int32), np.zeros(T)
    if T == 0:
        return dev, at, sumsq
    V = np.asarray(ev(np.ascontiguousarray(Q.reshape(-1, 3))), dtype=np.float64).reshape(T, S)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(S):
            v = V[:, s]
            take = np.full(T, True) if s == 0 else (dev == dev) & ((v != v) | (np.abs(v) > np.abs(dev)))
            dev = np.where(take, v, dev)
            at = np.where(take, np.int32(s), at).astype(np.int32)
            sumsq = sumsq + v * v
    return dev, at, sumsq


def snap(ev, P, eps, tol, max_move, iters):
    """(q (U, 3) float64, status (U,) uint8, residual (U,) float64, evals (U,) int32) of the points P (U, 3).  evals: the evaluations
    the vertex needed -- 1 per pass it entered, 6 more where it took the gradient, 1 for the final value of a vertex still ITER"""
    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), np.float64).reshape(-1) if len(Q) else np.zeros(0)

    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    U = len(P)
    eps, tol, max_move = np.float64(eps), np.float64(tol), np.float64(max_move)
    q = P.copy()
    status = np.full(U, _ITER, np.int32)
    evals = np.zeros(U, np.int32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for _ in range(int(iters)):
            m = np.flatnonzero(status == _ITER)
            if not len(m):
                break
            v = f(q[m])
            evals[m] += 1
            nan = v != v
            ok = ~nan & (np.abs(v) <= tol)
            status[m[nan]] = NAN
            q[m[nan]] = P[m[nan]]
            status[m[ok]] = SNAPPED
            go = ~nan & ~ok
            m, v = m[go], v[go]
            if not len(m):
                continue
            g = np.zeros((len(m), 3))
            for k in range(3):                           # as normals_ref.py: plus first, then minus
                plus = q[m].copy()
                plus[:, k] = q[m, k] + eps
                minus = q[m].copy()
                minus[:, k] = q[m, k] + (-eps)
                g[:, k] = f(plus) - f(minus)
            evals[m] += 6
            len2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            flat = (len2 == 0) | (len2 != len2)
            s = (v * (2 * eps)) / len2
            qn = q[m] - s[:, None] * g
            d = qn - P[m]
            far = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > max_move
            status[m[flat]] = FLAT
            status[m[~flat & far]] = HELD
            move = ~flat & ~far
            q[m[move]] = qn[move]
        residual = f(q)
        residual[status == NAN] = np.nan
        it = status == _ITER
        evals[it] += 1
        status[it & (np.abs(residual) <= tol)] = SNAPPED
        status[status == _ITER] = LEFT
    return q, status.astype(np.uint8), residual, evals


def lockstep_share(evals, iters, wave=64):
    """sum(evals) / the evaluations a kernel issues that runs `wave` vertices, in weld order, in lockstep: per run of `wave` vertices
    and per lane, the phases until no vertex of the run iterates -- the share of issued evaluations that a vertex still needed"""
    evals = np.asarray(evals)
    issued = sum(int(evals[i:i + wave].max()) for i in range(0, len(evals), wave)) * wave
    return float(evals.sum()) / issued if issued else 1.0
