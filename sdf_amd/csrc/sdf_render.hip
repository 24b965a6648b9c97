// sdf_render.hip -- sphere tracing of a model on the device (sdf_render_host, ABI 13): per pixel a ray is marched
// through the field by the tape interpreter until it comes within hit_eps of the surface, an overshoot is bisected back, and the
// normal is taken by central differences.  tests/render_ref.py is the definition; this kernel reproduces it bit for bit: float64, one
// rounding per written operation (-ffp-contract=off), divisions where the definition divides, dot = (x*x + y*y) + z*z.
//
// A wave takes an 8 x 8 PIXEL TILE (lane = 8 * row + column), a workgroup of 256 four tiles: the wave runs until its slowest ray is
// done, and neighbours in both directions march alike (DESIGN.md 4e has the shares).  One ray per lane.
//
// The interpreter is inlined ONCE: march, refinement and the six evaluations of the normal are phases of one loop whose phase and
// counter are wave-uniform (the march ends when `__any(status == MARCH)` says so or after max_steps passes, the others after `refine`
// and 6 passes).  Lanes never branch around the interpreter -- this unit is built with the structurizer option that is only safe for
// wave-uniform control flow (build.units) -- they take their state changes by selects: a lane that is done keeps evaluating at its frozen
// parameter and discards the value; a lane outside the image is a MISS from the start and stores nothing.
#include <cmath>
#include <string>

#include "sdf_interp.h"
#include "sdf_internal.h"

using namespace sdfk;

enum { R_MISS = 0, R_HIT = 1, R_MARCH = 2 };
enum { PH_MARCH = 0, PH_REFINE = 1, PH_NORMAL = 2 };

struct RenderArgs {
    double o0[3], ou[3], ov[3], c[3], du[3], dv[3];   // pixel (row j, column i): O = (o0 + i ou) + j ov, D = ((c + i du) + j dv) / |.|
    double t_near, t_far, hit_eps, step_scale, normal_eps;
    int width, height, tiles_x, n_tiles, max_steps, refine;
};

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
    double gp = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    int phase = PH_MARCH, k = 0;                                       // (wave-uniform, like every condition on them below)
    for (;;) {
        // the parameter along the ray this pass evaluates at: the march's t, the bisection's midpoint, the hit
        const double mid = 0.5 * (lo + hi);
        const double s = phase == PH_MARCH ? t : (phase == PH_REFINE ? mid : hi);
        double x = ox + s * dx, y = oy + s * dy, z = oz + s * dz;
        if (phase == PH_NORMAL) {                                      // pass k: axis k / 2, + h then - h
            const double h = (k & 1) ? -a.normal_eps : a.normal_eps;
            if ((k >> 1) == 0) x = x + h;
            else if ((k >> 1) == 1) y = y + h;
            else z = z + h;
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
            const double g = gp - v;
            if (k == 1) nx = g;
            else if (k == 3) ny = g;
            else if (k == 5) nz = g;
            gp = v;
            k++;
            if (k == 6) break;
        }
    }
    if (!inside) return;
    const bool is_hit = status == R_HIT;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool flat = len == 0.0 || len != len;
    const double qx = flat ? -dx : nx / len, qy = flat ? -dy : ny / len, qz = flat ? -dz : nz / len;
    const size_t p = (size_t)py * (size_t)a.width + (size_t)px;
    depth[p] = is_hit ? hi : (double)INFINITY;
    normal[3 * p] = is_hit ? qx : 0.0;
    normal[3 * p + 1] = is_hit ? qy : 0.0;
    normal[3 * p + 2] = is_hit ? qz : 0.0;
    steps_out[p] = steps;
    status_out[p] = is_hit ? 1 : 0;
}

static thread_local double g_render_kernel_ms = 0.0;

// 0: done, 1: HIP error, 2: refused (nothing allocated, nothing launched); sdf_last_error says why.  One device allocation, freed
// before it returns; sdf_render_last_kernel_ms: the kernel alone, by HIP events on the context's stream.
extern "C" int sdf_render_host(sdf_tape *t, const double *frame18, int width, int height, const double *params5, int max_steps, int refine,
                               double *h_depth, double *h_normal, int32_t *h_steps, uint8_t *h_status) {
    auto refuse = [](const std::string &why) { fail("sdf_render_host: " + why); return 2; };
    if (!t) return refuse("NULL argument");
    if (t->n_extern) return refuse("the tape reads user closures (L_EXTERN): every step of every ray would need a host round trip");
    HIPCHK(set_device(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    if (!t->d_code || !t->d_c64 || !frame18 || !params5 || !h_depth || !h_normal || !h_steps || !h_status) return refuse("NULL argument");
    if (width < 1 || height < 1) return refuse("empty image: " + std::to_string(width) + " x " + std::to_string(height));
    if ((long long)width * height > (1ll << 26)) return refuse("image of " + std::to_string(width) + " x " + std::to_string(height) + ": more than 2^26 pixels");
    if (max_steps < 1) return refuse("max_steps must be at least 1");
    if (refine < 0) return refuse("refine must not be negative");
    for (int i = 0; i < 18; i++) if (!std::isfinite(frame18[i])) return refuse("the ray frame is not finite");
    for (int i = 0; i < 5; i++) if (!std::isfinite(params5[i])) return refuse("the march parameters are not finite");
    const double t_near = params5[0], t_far = params5[1], hit_eps = params5[2], step_scale = params5[3], normal_eps = params5[4];
    if (!(hit_eps > 0.0)) return refuse("hit_eps must be positive");
    if (!(normal_eps > 0.0)) return refuse("normal_eps must be positive");
    if (!(step_scale > 0.0 && step_scale <= 1.0)) return refuse("step_scale must lie in (0, 1]");
    if (t_far < t_near) return refuse("t_far lies before t_near");

    RenderArgs a;
    for (int i = 0; i < 3; i++) {
        a.o0[i] = frame18[i]; a.ou[i] = frame18[3 + i]; a.ov[i] = frame18[6 + i];
        a.c[i] = frame18[9 + i]; a.du[i] = frame18[12 + i]; a.dv[i] = frame18[15 + i];
    }
    a.t_near = t_near; a.t_far = t_far; a.hit_eps = hit_eps; a.step_scale = step_scale; a.normal_eps = normal_eps;
    a.width = width; a.height = height; a.max_steps = max_steps; a.refine = refine;
    a.tiles_x = (width + 7) / 8;
    a.n_tiles = a.tiles_x * ((height + 7) / 8);                        // (at most 2^26 pixels: below 2^27 tiles even for a one-pixel-wide image)
    const size_t n = (size_t)width * (size_t)height;
    double *depth, *normal;
    int32_t *steps;
    uint8_t *status;
    Scratch scratch(st);
    scratch.part(&depth, n); scratch.part(&normal, 3 * n); scratch.part(&steps, n); scratch.part(&status, n);
    EventTimer timer;
    const unsigned grid = (unsigned)((a.n_tiles + 3) / 4);
    HIPCHK_FN(scratch.alloc());
    HIPCHK_FN(timer.start(st));
    LAUNCH_F64_ON(st, k_render, dim3(grid), dim3(256), 0, t->full, (const uint32_t *)t->d_code, (const double *)t->d_c64, a, depth, normal, steps, status);
    HIPCHK_FN(hipGetLastError());
    HIPCHK_FN(timer.stop(st));
    HIPCHK_FN(hipMemcpyAsync(h_depth, depth, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_normal, normal, n * 24, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_steps, steps, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_status, status, n, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(stream_wait(st));
    HIPCHK_FN(timer.ms(&g_render_kernel_ms));
    return 0;
}

extern "C" double sdf_render_last_kernel_ms(void) { return g_render_kernel_ms; }
