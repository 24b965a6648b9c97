// sdf_measure.h -- what measures a mesh on the device (sdf_measure.hip): the moments of a float64 soup and the
// edge census of an indexed mesh.  Both are synchronous on `st`, take their scratch in one hooked allocation that is back when they
// return, and return 0, or 1 with the message set.  *kernel_ms: their kernels alone, by HIP events.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdf_hip.h"
namespace sdfk {
// d_soup: n_tris x 9 float64 (n_tris >= 1); origin: 3 doubles on the host, or NULL for the midpoint of the soup's bounding box
int measure_moments(hipStream_t st, const double *d_soup, long long n_tris, const double *origin, sdf_moments *out, double *kernel_ms);
// d_cells: n_tris x 3 int64 vertex indices below n_vertices (n_tris >= 1, 3 n_tris < 2^31, n_vertices < 2^31)
int measure_edge_census(hipStream_t st, const long long *d_cells, long long n_tris, long long n_vertices, sdf_edge_census *out,
                        double *kernel_ms);
}
