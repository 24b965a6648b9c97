// sdf_thickness.h -- launcher of k_vertex_thickness (sdf_thickness.hip: a tape interpreter, built with the interpreters' flags).
// d_code / d_consts: a float64 tape on the device; full: it uses the trigonometric ops.  Enqueues on `st` and returns a hipError_t value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace sdfk {
struct ThicknessArgs {
    double normal_eps, start, min_step, t_far, step_scale;
    int max_steps, refine;
};
int launch_vertex_thickness(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                            const ThicknessArgs &a, double *d_thickness, uint8_t *d_status, int32_t *d_steps);
}
