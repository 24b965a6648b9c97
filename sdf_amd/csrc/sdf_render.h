// sdf_render.h -- launcher of k_render (sdf_render.hip: a tape interpreter, built with the interpreters' flags).  d_code / d_consts: a
// float64 tape on the device; full: it uses the trigonometric ops.  Enqueues on `st` and returns a hipError_t value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace sdfk {
struct RenderArgs {
    double o0[3], ou[3], ov[3], c[3], du[3], dv[3];   // pixel (row j, column i): O = (o0 + i ou) + j ov, D = ((c + i du) + j dv) / |.|
    double t_near, t_far, hit_eps, step_scale, normal_eps;
    int width, height, tiles_x, n_tiles, max_steps, refine;
};
int launch_render(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const RenderArgs &a, double *d_depth,
                  double *d_normal, int32_t *d_steps, uint8_t *d_status);
}
