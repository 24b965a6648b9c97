// sdf_deviation.h -- launchers of k_triangle_deviation and k_vertex_snap (sdf_deviation.hip: tape interpreters, built with the
// interpreters' flags).  d_code / d_consts: a float64 tape on the device; full: it uses the trigonometric ops.  Each enqueues on `st`
// and returns a hipError_t value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
namespace sdfk {
struct SnapArgs {
    double eps, two_eps, tol, max_move;
    int iters;
};
int launch_triangle_deviation(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_soup, long long n_tris,
                              int order, double *d_dev, int32_t *d_at, double *d_sumsq);
int launch_vertex_snap(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                       const SnapArgs &a, double *d_q, uint8_t *d_status, double *d_residual, int32_t *d_evals);
}
