// sdf_overhang.h -- what rates build directions on the device (sdf_overhang.hip): for a float64 soup and unit
// directions, the extremes along each direction and the three totals and two counts of tests/overhang_ref.py, and the class of every
// triangle for one direction.  (The unit also holds the driver and the plain kernels of the support rays, section 4o: they use these
// kernels as they are; see sdf_supports.h.)  Both follow the conventions of sdf_measure.h: synchronous on `st`, the scratch is one hooked
// allocation that is back when they return, and they return 0, or 1 with the message set.  *kernel_ms: their kernels alone, by HIP
// events.  The argument checks of the C ABI (unit directions, sin_limit in [0, 1), bed_tol >= 0) are the caller's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdfk {
constexpr long long OVERHANG_MAX_DIRS = 1ll << 20;
constexpr size_t OVERHANG_SCRATCH_CAP = (size_t)64 << 20;      // the default cap of the chunk partials of one slab of directions

// d_soup: n_tris x 9 float64 (1 <= n_tris < 2^31); h_dirs: n_dirs x 3 unit directions on the host (1 <= n_dirs <= 2^20).
// max_scratch_bytes: the cap of the chunk partials (0: OVERHANG_SCRATCH_CAP); the directions are taken in slabs that stay under it
// (a slab is never smaller than one direction) and no bit of the result depends on the slabs.  h_values: n_dirs x 5 (lo, hi, s0, s1,
// s2); h_counts: n_dirs x 2 (overhanging, bed-contact triangles); *n_slabs: how many slabs it took.
int overhang_rate(hipStream_t st, const double *d_soup, long long n_tris, const double *h_dirs, long long n_dirs, double sin_limit,
                  double bed_tol, size_t max_scratch_bytes, double *h_values, int64_t *h_counts, long long *n_slabs, double *kernel_ms);
// one direction h_dir3; h_classes: n_tris bytes on the host -- 0 neither, 1 overhang, 2 bed contact, 3 non-finite
int overhang_classes(hipStream_t st, const double *d_soup, long long n_tris, const double *h_dir3, double sin_limit, double bed_tol,
                     uint8_t *h_classes, double *kernel_ms);
}
