// sdf_render.hip -- sphere tracing of a model on the device (sdf_render_host, ABI 13): per pixel a ray is marched
// through the field by the tape interpreter until it comes within hit_eps of the surface, an overshoot is bisected back, and the
// normal is taken by central differences.  tests/render_ref.py is the definition; this kernel reproduces it bit for bit: float64, one
// rounding per written operation (-ffp-contract=off), divisions where the definition divides, dot = (x*x + y*y) + z*z.
//
// A wave takes an 8 x 8 PIXEL TILE (lane = 8 * row + column), a workgroup of 256 four tiles: the wave runs until its slowest ray is
// done, and neighbours in both directions march alike (DESIGN.md 4e has the shares).  One ray per lane.
//
// A probe kernel (sdf_probe.h has the doctrine), the phases MARCH -> REFINE -> NORMAL: the march ends when `__any(status == MARCH)`
// says so or after max_steps passes, the others after `refine` and 6 passes.  A lane that is done evaluates at its frozen parameter;
// a lane outside the image is a MISS from the start and stores nothing.
#include <cmath>

#include "sdf_interp.h"
#include "sdf_probe.h"
#include "sdf_render.h"

using namespace sdfk;

enum { R_MISS = 0, R_HIT = 1, R_MARCH = 2 };
enum { PH_MARCH = 0, PH_REFINE = 1, PH_NORMAL = 2 };

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_render(const uint32_t *__restrict__ code, const T *__restrict__ consts, const RenderArgs a,
                                                double *__restrict__ depth, double *__restrict__ normal, int32_t *__restrict__ steps_out,
                                                uint8_t *__restrict__ status_out) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;                                     // (wave-uniform)
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
    const bool inside = px < a.width && py < a.height;
    const double fi = (double)px, fj = (double)py;
    const double ox = (a.o0[0] + fi * a.ou[0]) + fj * a.ov[0], oy = (a.o0[1] + fi * a.ou[1]) + fj * a.ov[1], oz = (a.o0[2] + fi * a.ou[2]) + fj * a.ov[2];
    double dx = (a.c[0] + fi * a.du[0]) + fj * a.dv[0], dy = (a.c[1] + fi * a.du[1]) + fj * a.dv[1], dz = (a.c[2] + fi * a.du[2]) + fj * a.dv[2];
    {
        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
        dx = dx / len; dy = dy / len; dz = dz / len;
    }
    double t = a.t_near, lo = a.t_near, hi = a.t_near;
    int status = inside ? R_MARCH : R_MISS, steps = 0;
    bool neg = false, fix = false;
    Grad g = {0.0, 0.0, 0.0, 0.0};
    int phase = PH_MARCH, k = 0;                                       // (wave-uniform, like every condition on them below)
    for (;;) {
        // the parameter along the ray this pass evaluates at: the march's t, the bisection's midpoint, the hit
        const double mid = 0.5 * (lo + hi);
        const double s = phase == PH_MARCH ? t : (phase == PH_REFINE ? mid : hi);
        double x = ox + s * dx, y = oy + s * dy, z = oz + s * dz;
        if (phase == PH_NORMAL) {
            const P3 p = grad_point(k, a.normal_eps, x, y, z);
            x = p.x; y = p.y; z = p.z;
        }
        const double v = (double)run_tape1<T, FULL>(code, consts, (T)x, (T)y, (T)z);
        if (phase == PH_MARCH) {
            const bool m = status == R_MARCH;
            const bool nan = v != v, hit = !nan && v < a.hit_eps, go = !nan && !hit;
            const double t1 = t + v * a.step_scale;
            steps += m ? 1 : 0;
            hi = (m && hit) ? t : hi;
            neg = (m && hit) ? v < 0.0 : neg;
            lo = (m && go) ? t : lo;
            t = (m && go) ? t1 : t;
            status = !m ? status : (nan ? R_MISS : (hit ? R_HIT : (t1 > a.t_far ? R_MISS : R_MARCH)));
            k++;
            if (!(__any(status == R_MARCH) && k < a.max_steps)) {
                status = status == R_MARCH ? R_MISS : status;          // ran out of steps
                if (!__any(status == R_HIT)) break;                    // a tile of misses: nothing to refine, no normal to take
                fix = status == R_HIT && neg && steps > 1;
                phase = (a.refine > 0 && __any(fix)) ? PH_REFINE : PH_NORMAL;
                k = 0;
            }
        } else if (phase == PH_REFINE) {
            const bool in = v < 0.0;
            hi = (fix && in) ? mid : hi;
            lo = (fix && !in) ? mid : lo;
            k++;
            if (k == a.refine) { phase = PH_NORMAL; k = 0; }
        } else {
            g = grad_take(g, k, v);
            k++;
            if (k == 6) break;
        }
    }
    if (!inside) return;
    const bool is_hit = status == R_HIT;
    const double len = sqrt(grad_len2(g.g0, g.g1, g.g2));
    const bool flat = grad_flat(len);
    const double qx = flat ? -dx : g.g0 / len, qy = flat ? -dy : g.g1 / len, qz = flat ? -dz : g.g2 / len;
    const size_t p = (size_t)py * (size_t)a.width + (size_t)px;
    depth[p] = is_hit ? hi : (double)INFINITY;
    normal[3 * p] = is_hit ? qx : 0.0;
    normal[3 * p + 1] = is_hit ? qy : 0.0;
    normal[3 * p + 2] = is_hit ? qz : 0.0;
    steps_out[p] = steps;
    status_out[p] = is_hit ? 1 : 0;
}

namespace sdfk {

// enqueue only: the image of a.width x a.height >= 1 pixels (a.tiles_x, a.n_tiles filled in) into d_depth / d_normal / d_steps /
// d_status.  Returns a hipError_t value (0 = ok).
int launch_render(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const RenderArgs &a, double *d_depth,
                  double *d_normal, int32_t *d_steps, uint8_t *d_status) {
    const unsigned grid = (unsigned)((a.n_tiles + 3) / 4);
    LAUNCH_F64_ON(st, k_render, dim3(grid), dim3(256), 0, full, d_code, d_consts, a, d_depth, d_normal, d_steps, d_status);
    return (int)hipGetLastError();
}

}  // namespace sdfk
