// sdf_measure.h -- what measures a mesh on the device (sdf_measure.hip): the moments of a float64 soup and the
// edge census of an indexed mesh.  Both are synchronous on `st`, take their scratch in one hooked allocation that is back when they
// return, and return 0, or 1 with the message set.  *kernel_ms: their kernels alone, by HIP events.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdf_hip.h"
namespace sdfk {
// the keys of a bounding box that integer atomics can take (k_soup_box here, the shells' boxes of sdf_components.hip):
// float64 -> u64 whose unsigned order is the float order; both zeros give the key of +0.0
__device__ __forceinline__ unsigned long long box_key(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __host__ __forceinline__ unsigned long long box_bits(unsigned long long k) { return (k >> 63) ? (k & ~(1ull << 63)) : ~k; }
// the empty box: every lower bound is the key of +inf, every upper bound the key of -inf
constexpr unsigned long long BOX_EMPTY_LO = 0xfff0000000000000ull, BOX_EMPTY_HI = ~BOX_EMPTY_LO;

// d_soup: n_tris x 9 float64 (n_tris >= 1); origin: 3 doubles on the host, or NULL for the midpoint of the soup's bounding box
int measure_moments(hipStream_t st, const double *d_soup, long long n_tris, const double *origin, sdf_moments *out, double *kernel_ms);
// d_cells: n_tris x 3 int64 vertex indices below n_vertices (n_tris >= 1, 3 n_tris < 2^31, n_vertices < 2^31)
int measure_edge_census(hipStream_t st, const long long *d_cells, long long n_tris, long long n_vertices, sdf_edge_census *out,
                        double *kernel_ms);
}
