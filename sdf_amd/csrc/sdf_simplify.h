// sdf_simplify.h -- a welded mesh simplified on the device (sdf_simplify.hip): vertex clustering on a uniform
// grid, one quadric-placed representative per cluster, the surviving triangles as a soup of its own.  Synchronous on `st`; the
// scratch is one hooked allocation that is back when the call returns; 0, or 1 with the message set.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdf_hip.h"
#include "sdf_runtime.h"
namespace sdfk {
// d_points: n_vertices x 3 float64 and d_cells: n_tris x 3 int64 indices below n_vertices (the weld's; 1 <= n_vertices, 3 n_tris <
// 2^31); origin, cell: 3 doubles on the host, finite, cell > 0; reg >= 0.  The survivors go into `out` (grown as needed; left alone
// when none survives).  A vertex that is not finite, or clusters that span 2^21 or more cells on an axis, are found after the first
// pass and fail the call before anything is written to `out`.  kernel_ms[0..3]: keys and numbering, the item sort and its segments,
// k_cluster_vertex, live flags and emission, by HIP events; stats->kernel_ms is their sum.
int simplify_device(hipStream_t st, const double *d_points, const long long *d_cells, long long n_vertices, long long n_tris,
                    const double *origin, const double *cell, double reg, DevBuf *out, sdf_simplify_stats *stats, double kernel_ms[4]);
// The same mesh simplified to a tolerance: the levels 0 .. levels (<= SDF_ADAPTIVE_MAX_LEVELS) of cell x 2^L,
// every one finite, from the coarsest down in one scratch; tolerance >= 0, +inf allowed.  level_ms[0 .. levels]: the kernels of
// every level, *emit_ms: live flags and emission, by HIP events; stats->kernel_ms is their sum.  Fails like simplify_device, before
// anything is written to `out`.
int simplify_adaptive_device(hipStream_t st, const double *d_points, const long long *d_cells, long long n_vertices, long long n_tris,
                             const double *origin, const double *cell, double reg, double tolerance, int levels, DevBuf *out,
                             sdf_adaptive_stats *stats, double *level_ms, double *emit_ms);
}
