// sdf_mend.h -- a welded mesh mended on the device (sdf_mend.hip): duplicate triangles dropped, oppositely
// wound pairs cancelled, the survivors as a soup of its own.  Synchronous on `st`; the scratch is one hooked allocation that is back
// when the call returns; 0, or 1 with the message set.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdf_hip.h"
#include "sdf_runtime.h"
namespace sdfk {
// d_soup: n_tris x 9 float64, the soup the weld was taken of, and d_cells: n_tris x 3 int64 indices below n_vertices (the weld's;
// 1 <= n_vertices < 2^31, 1 <= 3 n_tris < 2^31).  The survivors' nine doubles go from d_soup into `out`, in soup order (grown as
// needed; left alone when none survives).  kernel_ms[0..2]: the keys, the two sorts, runs and emission, by HIP events;
// stats->kernel_ms is their sum.
int mend_device(hipStream_t st, const double *d_soup, const long long *d_cells, long long n_vertices, long long n_tris, DevBuf *out,
                sdf_mend_stats *stats, double kernel_ms[3]);
}
