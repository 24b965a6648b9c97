// sdf_normals.h -- launcher of k_vertex_normals (sdf_normals.hip: a tape interpreter, built with the interpreters' flags).  d_code /
// d_consts: a float64 tape on the device; full: it uses the trigonometric ops.  Enqueues on `st` and returns a hipError_t value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace sdfk {
int launch_vertex_normals(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                          double eps, double *d_out, unsigned long long *d_flat);
}
