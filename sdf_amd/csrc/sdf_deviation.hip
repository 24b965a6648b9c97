// sdf_deviation.hip -- a mesh held to the field it came from (sdf_mesh_triangle_deviation, sdf_mesh_snap): how far
// every triangle of the soup lies from the zero set, sampled on a barycentric lattice, and the welded vertices put back on the zero
// set by Newton steps along the field's gradient.  tests/deviation_ref.py is the definition; these kernels reproduce it bit for bit
// over the interpreter that sdf_eval_points runs: float64, one rounding per written operation (-ffp-contract=off), divisions where the
// definition divides, dot = (x*x + y*y) + z*z, a sample point is (A*wa + B*wb) + C*wc, a Newton step is q - s * g.
//
// Two probe kernels (sdf_probe.h has the doctrine).  k_triangle_deviation: one triangle of the float64 soup per lane (no weld, like
// the moments), one phase -- the samples of the lattice.  k_vertex_snap: one welded vertex per lane, the phases value -> six gradient
// passes -> value -> ... -> final value, left early when `__any(status == ITER)` says no lane has work; a lane that is done evaluates
// at its frozen point.
#include <cmath>

#include "sdf_interp.h"
#include "sdf_deviation.h"
#include "sdf_probe.h"

using namespace sdfk;

enum { S_LEFT = 0, S_SNAPPED = 1, S_HELD = 2, S_FLAT = 3, S_NAN = 4, S_ITER = 5 };     // (0 .. 4: the status codes of the ABI)

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_triangle_deviation(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                            const double *__restrict__ soup, long long n, int order,
                                                            double *__restrict__ dev_out, int32_t *__restrict__ at_out,
                                                            double *__restrict__ sumsq_out) {
    const long long wave0 = (long long)blockIdx.x * 256 + (long long)(threadIdx.x & ~63u);
    if (wave0 >= n) return;                                            // (wave-uniform)
    const long long t = wave0 + (long long)(threadIdx.x & 63u);
    const bool live = t < n;
    const double *__restrict__ tri = soup + 9 * (live ? t : n - 1);
    const double ax = tri[0], ay = tri[1], az = tri[2];
    const double bx = tri[3], by = tri[4], bz = tri[5];
    const double cx = tri[6], cy = tri[7], cz = tri[8];
    const double dn = (double)order;
    const int n_samples = (order + 1) * (order + 2) / 2;
    double dev = 0.0, sumsq = 0.0;
    int at = 0;
    int i = 0, j = 0;                                                  // (wave-uniform, like every condition on them below)
#pragma unroll 1
    for (int s = 0; s < n_samples; s++) {                              // for i in 0 .. n: for j in 0 .. n - i
        const double wa = (double)(order - i - j) / dn, wb = (double)i / dn, wc = (double)j / dn;
        const double x = (ax * wa + bx * wb) + cx * wc;
        const double y = (ay * wa + by * wb) + cy * wc;
        const double z = (az * wa + bz * wb) + cz * wc;
        const double v = (double)run_tape1<T, FULL>(code, consts, (T)x, (T)y, (T)z);
        // the value of largest magnitude: strictly greater replaces, the first NaN replaces and stays
        const bool take = s == 0 || (dev == dev && (v != v || fabs(v) > fabs(dev)));
        dev = take ? v : dev;
        at = take ? s : at;
        sumsq = sumsq + v * v;
        j++;
        if (j > order - i) { i++; j = 0; }
    }
    if (!live) return;
    dev_out[t] = dev;
    at_out[t] = at;
    sumsq_out[t] = sumsq;
}

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_vertex_snap(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                     const double *__restrict__ pts, long long n, const SnapArgs a,
                                                     double *__restrict__ q_out, uint8_t *__restrict__ status_out,
                                                     double *__restrict__ residual_out, int32_t *__restrict__ evals_out) {
    const long long wave0 = (long long)blockIdx.x * 256 + (long long)(threadIdx.x & ~63u);
    if (wave0 >= n) return;                                            // (wave-uniform)
    const long long i = wave0 + (long long)(threadIdx.x & 63u);
    const bool live = i < n;
    const long long l = live ? i : n - 1;
    const double px = pts[3 * l], py = pts[3 * l + 1], pz = pts[3 * l + 2];
    double qx = px, qy = py, qz = pz;
    Grad g = {0.0, 0.0, 0.0, 0.0};
    double v0 = 0.0, res = 0.0;
    int status = S_ITER, evals = 0;
    int pass = 0, k = 0;                                               // (wave-uniform, like every condition on them below)
    for (;;) {
        // where this phase evaluates: q (k = 0), or gradient pass k - 1 around q
        double x = qx, y = qy, z = qz;
        if (k > 0) {
            const P3 p = grad_point(k - 1, a.eps, qx, qy, qz);
            x = p.x; y = p.y; z = p.z;
        }
        const double v = (double)run_tape1<T, FULL>(code, consts, (T)x, (T)y, (T)z);
        const bool it = status == S_ITER;
        if (k == 0) {
            evals += it ? 1 : 0;
            if (pass == a.iters) {                                     // the passes are over: the residual of what still iterates
                res = it ? v : res;
                status = it ? (fabs(v) <= a.tol ? S_SNAPPED : S_LEFT) : status;
                break;
            }
            const bool nan = v != v, ok = !nan && fabs(v) <= a.tol;
            res = it ? (nan ? (double)NAN : v) : res;                  // (a lane that stops here or below stays where v was taken)
            v0 = v;
            qx = (it && nan) ? px : qx;
            qy = (it && nan) ? py : qy;
            qz = (it && nan) ? pz : qz;
            status = !it ? status : (nan ? S_NAN : (ok ? S_SNAPPED : S_ITER));
            if (!__any(status == S_ITER)) break;
            k = 1;
        } else {
            const double d = g.gp - v;                                 // (grad_take spelt out: through the helper this kernel compiles to
            if (k == 2) g.g0 = d;                                      // other instructions, profiles/probe_spine_refactor.md)
            else if (k == 4) g.g1 = d;
            else if (k == 6) g.g2 = d;
            g.gp = v;
            if (k == 6) {
                evals += it ? 6 : 0;
                const double len2 = grad_len2(g.g0, g.g1, g.g2);
                const bool flat = grad_flat(len2);
                const double s = (v0 * a.two_eps) / len2;              // the Newton step v * grad / |grad|^2
                const double nx = qx - s * g.g0, ny = qy - s * g.g1, nz = qz - s * g.g2;
                const double dx = nx - px, dy = ny - py, dz = nz - pz;
                const bool far = sqrt((dx * dx + dy * dy) + dz * dz) > a.max_move;
                const bool move = it && !flat && !far;
                status = !it ? status : (flat ? S_FLAT : (far ? S_HELD : S_ITER));
                qx = move ? nx : qx;
                qy = move ? ny : qy;
                qz = move ? nz : qz;
                pass++;
                k = 0;
                if (!__any(status == S_ITER)) break;
            } else {
                k++;
            }
        }
    }
    if (!live) return;
    q_out[3 * i] = qx;
    q_out[3 * i + 1] = qy;
    q_out[3 * i + 2] = qz;
    status_out[i] = (uint8_t)status;
    residual_out[i] = res;
    evals_out[i] = evals;
}

namespace sdfk {

// enqueue only: the deviation of n_tris >= 1 triangles (n_tris x 9 float64 at d_soup), order 1 .. 8, into d_dev / d_at / d_sumsq.
// Returns a hipError_t value (0 = ok).
int launch_triangle_deviation(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_soup, long long n_tris,
                              int order, double *d_dev, int32_t *d_at, double *d_sumsq) {
    if (n_tris < 1) return 0;
    const unsigned grid = (unsigned)((n_tris + 255) / 256);            // (the callers refuse 2^31 triangles and more)
    LAUNCH_F64_ON(st, k_triangle_deviation, dim3(grid), dim3(256), 0, full, d_code, d_consts, d_soup, n_tris, order, d_dev, d_at, d_sumsq);
    return (int)hipGetLastError();
}

// enqueue only: n >= 1 vertices (n x 3 float64 at d_pts) snapped into d_q (n x 3), with d_status / d_residual / d_evals.  Returns a
// hipError_t value (0 = ok).
int launch_vertex_snap(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                       const SnapArgs &a, double *d_q, uint8_t *d_status, double *d_residual, int32_t *d_evals) {
    if (n < 1) return 0;
    const unsigned grid = (unsigned)((n + 255) / 256);                 // (n < 2^31 vertices: the weld's limit)
    LAUNCH_F64_ON(st, k_vertex_snap, dim3(grid), dim3(256), 0, full, d_code, d_consts, d_pts, n, a, d_q, d_status, d_residual, d_evals);
    return (int)hipGetLastError();
}

}  // namespace sdfk
