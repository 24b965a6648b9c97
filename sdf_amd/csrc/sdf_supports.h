// sdf_supports.h -- support rays traced through the field (tests/supports_ref.py is the definition).  Two halves:
// the launcher of k_support_rays (sdf_supports.hip: a tape interpreter, built with the interpreters' flags), and the driver of one call
// (sdf_overhang.hip: plain kernels -- the classes and extents of section 4n, the numbering of the overhanging faces, the ordered sums).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "sdf_runtime.h"

namespace sdfk {
constexpr int SUPPORT_SUMS = 5;                    // tests/supports_ref.py: the five term columns
constexpr int SUPPORT_STATUSES = 5;                // BED, PART, BURIED, UNRESOLVED, NAN
constexpr long long SUPPORT_MAX_DIRS = 1024;

struct SupportArgs {
    double dx, dy, dz, lo;                         // the unit direction "up" and the bed plane's height along it
    double start, min_step, step_scale;
    int max_steps, refine;
};

// enqueue only: the rays of the m >= 1 triangles d_triangle[0 .. m) of the float64 soup.  d_code / d_consts: a float64 tape on the
// device; full: it uses the trigonometric ops.  d_origin: m x 3; d_terms: SUPPORT_SUMS columns of m (column c at d_terms + c * m).
// Returns a hipError_t value (0 = ok).
int launch_support_rays(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_soup,
                        const int32_t *d_triangle, long long m, const SupportArgs &a, double *d_height, uint8_t *d_status, int32_t *d_steps,
                        double *d_origin, double *d_terms);

// what one direction leaves on the device: one block of origin (m x 3 float64), height (m float64), triangle, steps (m int32 each),
// status (m bytes), in that order at the offsets below; no block where m == 0
struct SupportRaysDir {
    DevBlock block;
    long long m = 0;
    size_t o_height = 0, o_triangle = 0, o_steps = 0, o_status = 0;
};

struct SupportParams {
    double sin_limit, bed_tol, start, min_step, step_scale;
    int max_steps, refine;
};

// The directions one after another on `st` (1 <= n_tris < 2^31, 1 <= n_dirs <= SUPPORT_MAX_DIRS, h_dirs: unit directions on the
// host): per direction the classes and extents of sdf_overhang.hip, the overhanging faces numbered (one wait for their count), their
// rays, the five sums through the fixed tree over the rays and the status counts.  One hooked scratch block for the call, sized once;
// one block per direction with rays in `out`.  h_values: n_dirs x 7 (lo, hi, s0 .. s4); h_counts: n_dirs x 6 (the five statuses, m).
// parts_ms4: classes + extents, numbering, rays, sums -- kernels alone, by HIP events, summed over the directions.  Synchronous;
// returns 0, or 1 with the message set and nothing left allocated but what `out` holds (the caller drops it).
int support_rays_run(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_soup, long long n_tris,
                     const double *h_dirs, long long n_dirs, const SupportParams &p, std::vector<SupportRaysDir> *out, double *h_values,
                     int64_t *h_counts, double *parts_ms4);
}
