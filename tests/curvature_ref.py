"""The definition of the curvature probe, in NumPy over an evaluator `ev(P) -> (N,) float64` that the caller
passes: the CPU checker (`oracle.evaluate`), the device interpreter (`Engine.eval_points`) or an analytic field.
csrc/sdf_curvature.hip (k_vertex_curvature) reproduces it bit for bit, sdf_amd/curvature.py (`vertex_curvature`) restates it for
the host path.

The mean and the Gaussian curvature of the level set of the field f through a point p are closed forms in the gradient G and the
Hessian H of f there; both are taken from second differences of f at step eps: 19 values per point.

All arithmetic is float64 with one rounding per written operation: a product and a sum are two operations, a quotient is a division,
products of three factors are taken left to right.  A coordinate is moved as `x + eps` and `x + (-eps)` (csrc/sdf_probe.h,
grad_point).  The field is negative inside, so convex is positive: `sphere(R)` has k1 = k2 = 1 / R, a cavity is negative."""
import numpy as np

CURVED, FLAT, NAN = 0, 1, 2
NAMES = ('CURVED', 'FLAT', 'NAN')
PASSES = 19
PAIRS = ((0, 1), (0, 2), (1, 2))                       # the axis pairs of the mixed differences: (x, y), (x, z), (y, z)
CORNERS = ((1, 1), (1, -1), (-1, 1), (-1, -1))         # the corners of a pair: ++, +-, -+, --
NAN_BITS = 0x7ff8000000000000                          # np.nan's: what a vertex without a curvature holds, by a select


def bits(a):
    """the bit patterns of an array (float64 -> int64): what 'bit for bit' compares"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def stencil(P, k, eps):
    """where pass k = 0 .. 18 evaluates: 0 the points themselves; 1 .. 6 axis (k - 1) // 2 moved by + eps (k odd) or + (-eps);
    7 .. 18 the pair PAIRS[(k - 7) // 4], its first axis moved by +-eps, then its second, in the order of CORNERS"""
    Q = P.copy()
    if 1 <= k <= 6:
        a = (k - 1) // 2
        Q[:, a] = P[:, a] + (eps if (k - 1) % 2 == 0 else -eps)
    elif k >= 7:
        a, b = PAIRS[(k - 7) // 4]
        sa, sb = CORNERS[(k - 7) % 4]
        Q[:, a] = P[:, a] + (eps if sa > 0 else -eps)
        Q[:, b] = P[:, b] + (eps if sb > 0 else -eps)
    return Q


def curvature(ev, P, eps, debug=False):
    """(curv (U, 4) float64: mean, gauss, k1, k2; status (U,) uint8) at the points P (U, 3); with debug=True a third value: a dict of
    `values` (19, U), `G` (3, U), `H` (6, U: xx, yy, zz, xy, xz, yz)"""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    U = len(P)
    eps = np.float64(eps)

    def f(Q):
        return np.asarray(ev(np.ascontiguousarray(Q)), np.float64).reshape(-1) if U else np.zeros(0)

    with np.errstate(all='ignore'):
        v = [f(stencil(P, k, eps)) for k in range(PASSES)]
        v0 = v[0]
        two_eps, eps2, four_eps2 = 2 * eps, eps * eps, (4 * eps) * eps
        Gx, Gy, Gz = [(v[1 + 2 * a] - v[2 + 2 * a]) / two_eps for a in range(3)]
        Hxx, Hyy, Hzz = [((v[1 + 2 * a] - v0) + (v[2 + 2 * a] - v0)) / eps2 for a in range(3)]
        Hxy, Hxz, Hyz = [((v[7 + 4 * p] - v[8 + 4 * p]) - (v[9 + 4 * p] - v[10 + 4 * p])) / four_eps2 for p in range(3)]

        L2 = (Gx * Gx + Gy * Gy) + Gz * Gz
        L = np.sqrt(L2)
        tr = (Hxx + Hyy) + Hzz
        gHg = ((Gx * Gx * Hxx + Gy * Gy * Hyy) + Gz * Gz * Hzz) + 2 * ((Gx * Gy * Hxy + Gx * Gz * Hxz) + Gy * Gz * Hyz)
        mean = (L2 * tr - gHg) / ((2 * L2) * L)
        Axx = Hyy * Hzz - Hyz * Hyz
        Ayy = Hxx * Hzz - Hxz * Hxz
        Azz = Hxx * Hyy - Hxy * Hxy
        Axy = Hxz * Hyz - Hxy * Hzz
        Axz = Hxy * Hyz - Hxz * Hyy
        Ayz = Hxy * Hxz - Hxx * Hyz
        gAg = ((Gx * Gx * Axx + Gy * Gy * Ayy) + Gz * Gz * Azz) + 2 * ((Gx * Gy * Axy + Gx * Gz * Axz) + Gy * Gz * Ayz)
        gauss = gAg / (L2 * L2)
        disc = mean * mean - gauss
        disc = np.where(disc > 0, disc, 0.0)
        s = np.sqrt(disc)
        k1 = mean + s
        k2 = mean - s

    bad = np.zeros(U, bool)
    for k in range(PASSES):
        bad |= ~np.isfinite(v[k])
    flat = (L2 == 0) | ~np.isfinite(L)
    broken = ~(np.isfinite(mean) & np.isfinite(gauss) & np.isfinite(k1) & np.isfinite(k2))
    status = np.where(bad, NAN, np.where(flat, FLAT, np.where(broken, NAN, CURVED))).astype(np.uint8)
    curv = np.stack([mean, gauss, k1, k2], axis=1) if U else np.zeros((0, 4))
    curv = np.ascontiguousarray(curv, dtype=np.float64)
    curv.view(np.uint64)[status != CURVED] = NAN_BITS
    if debug:
        return curv, status, {'values': np.array(v), 'G': np.array([Gx, Gy, Gz]), 'H': np.array([Hxx, Hyy, Hzz, Hxy, Hxz, Hyz])}
    return curv, status


def counts(status):
    """the status histogram as the device counts it: (CURVED, FLAT, NAN) int64"""
    return np.bincount(np.asarray(status, dtype=np.uint8), minlength=3).astype(np.int64)
