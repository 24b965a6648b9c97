// sdf_curvature.h -- launcher of k_vertex_curvature (sdf_curvature.hip: a tape interpreter, built with the interpreters' flags).  d_code /
// d_consts: a float64 tape on the device; full: it uses the trigonometric ops.  Enqueues on `st` and returns a hipError_t value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace sdfk {
int launch_vertex_curvature(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                            double eps, double *d_out4, uint8_t *d_status, unsigned long long *d_counts3);
}
