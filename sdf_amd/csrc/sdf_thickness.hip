// sdf_thickness.hip -- the wall thickness at the welded vertices of a mesh (sdf_mesh_vertex_thickness): from every
// vertex a ray is sphere-traced INWARD, along the negated field normal, through the solid until the field turns positive again; the
// bracket of that crossing is bisected and the ray's length is the wall's ray thickness there.  tests/thickness_ref.py is the
// definition; this kernel reproduces it bit for bit over the interpreter that sdf_eval_points runs: float64, one rounding per written
// operation (-ffp-contract=off), divisions where the definition divides, dot = (x*x + y*y) + z*z, a point on a ray is p + t * d.
//
// A probe kernel (sdf_probe.h has the doctrine): one welded vertex per lane, the phases NORMAL -> MARCH -> REFINE: the march ends
// when `__any(status == MARCH)` says so or after max_steps passes, REFINE is skipped when no lane of the wave is THICK.  A lane that
// is done evaluates at its frozen parameter, a FLAT lane (direction 0) at its vertex.
#include <cmath>

#include "sdf_interp.h"
#include "sdf_probe.h"
#include "sdf_thickness.h"

using namespace sdfk;

enum { W_OPEN = 0, W_THICK = 1, W_THIN = 2, W_FLAT = 3, W_NAN = 4, W_MARCH = 5 };      // (0 .. 4: the status codes of the ABI)
enum { PH_NORMAL = 0, PH_MARCH = 1, PH_REFINE = 2 };

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_vertex_thickness(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                          const double *__restrict__ pts, long long n, const ThicknessArgs a,
                                                          double *__restrict__ thickness, uint8_t *__restrict__ status_out,
                                                          int32_t *__restrict__ steps_out) {
    const long long wave0 = (long long)blockIdx.x * 256 + (long long)(threadIdx.x & ~63u);
    if (wave0 >= n) return;                                            // (wave-uniform)
    const long long i = wave0 + (long long)(threadIdx.x & 63u);
    const bool live = i < n;
    const long long j = live ? i : n - 1;
    const double px = pts[3 * j], py = pts[3 * j + 1], pz = pts[3 * j + 2];
    Grad g = {0.0, 0.0, 0.0, 0.0};
    double dx = 0.0, dy = 0.0, dz = 0.0;
    double t = a.start, lo = 0.0, hi = a.start;
    int status = W_MARCH, steps = 0;
    int phase = PH_NORMAL, k = 0;                                      // (wave-uniform, like every condition on them below)
    for (;;) {
        // where this pass evaluates: the vertex moved by +-eps along an axis, the march's t, the bisection's midpoint
        const double mid = 0.5 * (lo + hi);
        const bool fix = status == W_THICK;
        const double s = (phase == PH_REFINE && fix) ? mid : t;
        double x = px + s * dx, y = py + s * dy, z = pz + s * dz;
        if (phase == PH_NORMAL) {
            const P3 p = grad_point(k, a.normal_eps, px, py, pz);
            x = p.x; y = p.y; z = p.z;
        }
        const double v = (double)run_tape1<T, FULL>(code, consts, (T)x, (T)y, (T)z);
        if (phase == PH_NORMAL) {
            const double d = g.gp - v;                                 // (grad_take spelt out: through the helper this kernel compiles to
            if (k == 1) g.g0 = d;                                      // other instructions, profiles/probe_spine_refactor.md)
            else if (k == 3) g.g1 = d;
            else if (k == 5) g.g2 = d;
            g.gp = v;
            k++;
            if (k == 6) {
                const double len = sqrt(grad_len2(g.g0, g.g1, g.g2));
                const bool flat = grad_flat(len);
                dx = flat ? 0.0 : -(g.g0 / len);                       // inward for this library's winding
                dy = flat ? 0.0 : -(g.g1 / len);
                dz = flat ? 0.0 : -(g.g2 / len);
                status = flat ? W_FLAT : W_MARCH;
                if (!__any(status == W_MARCH)) break;                  // a wave of flat vertices: no ray to march
                phase = PH_MARCH; k = 0;
            }
        } else if (phase == PH_MARCH) {
            const bool m = status == W_MARCH;
            const bool nan = v != v, out = !nan && v >= 0.0, in = !nan && !out;
            const double adv = (-v) * a.step_scale;
            const double t1 = t + (adv > a.min_step ? adv : a.min_step);
            const bool far = t1 > a.t_far;
            steps += m ? 1 : 0;
            hi = (m && out) ? t : hi;
            lo = (m && in) ? t : lo;
            status = !m ? status : (nan ? W_NAN : (out ? (k == 0 ? W_THIN : W_THICK) : (far ? W_OPEN : W_MARCH)));
            t = (m && in && !far) ? t1 : t;
            k++;
            if (!(__any(status == W_MARCH) && k < a.max_steps)) {
                status = status == W_MARCH ? W_OPEN : status;          // ran out of steps
                if (!(a.refine > 0 && __any(status == W_THICK))) break;
                phase = PH_REFINE; k = 0;
            }
        } else {
            const bool in = v < 0.0;
            lo = (fix && in) ? mid : lo;
            hi = (fix && !in) ? mid : hi;                              // (NaN included)
            k++;
            if (k == a.refine) break;
        }
    }
    if (!live) return;
    thickness[i] = (status == W_THICK || status == W_THIN) ? hi : (status == W_OPEN ? (double)INFINITY : (double)NAN);
    status_out[i] = (uint8_t)status;
    steps_out[i] = steps;
}

namespace sdfk {

// enqueue only: the thickness of n >= 1 vertices (n x 3 float64 at d_pts) into d_thickness / d_status / d_steps.  Returns a
// hipError_t value (0 = ok).
int launch_vertex_thickness(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                            const ThicknessArgs &a, double *d_thickness, uint8_t *d_status, int32_t *d_steps) {
    if (n < 1) return 0;
    const unsigned grid = (unsigned)((n + 255) / 256);                 // (n < 2^31 vertices: the weld's limit)
    LAUNCH_F64_ON(st, k_vertex_thickness, dim3(grid), dim3(256), 0, full, d_code, d_consts, d_pts, n, a, d_thickness, d_status, d_steps);
    return (int)hipGetLastError();
}

}  // namespace sdfk
