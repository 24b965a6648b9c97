// sdf_curvature.hip -- the curvature of the field's level set at the welded vertices of a mesh (sdf_mesh_vertex_curvature; DESIGN.md
// section 4t): mean, Gaussian and the two principal curvatures, closed forms in the gradient G and the Hessian H of the field, both
// taken from second differences at step eps.  tests/curvature_ref.py is the definition; this kernel reproduces it bit for bit over
// the interpreter that sdf_eval_points runs: float64, one rounding per written operation (-ffp-contract=off), divisions where the
// definition divides, products of three factors left to right.
//
// A probe kernel (sdf_probe.h has the doctrine): one welded vertex per lane, one phase -- 19 passes: the vertex, the six points of
// the central difference (grad_point), the four corners of the axis pairs (x, y), (x, z), (y, z).  Every value is folded into its
// accumulator as it arrives: v0, G (3), the diagonal of H (3), its off-diagonal (3) and two temporaries live across the interpreter,
// not 19 values.  The statuses are counted by one integer atomic add per wave that has any.
#include <cmath>

#include "sdf_interp.h"
#include "sdf_curvature.h"
#include "sdf_probe.h"

using namespace sdfk;

enum { C_CURVED = 0, C_FLAT = 1, C_NAN = 2 };                          // (the status codes of the ABI)

// pass m = 0 .. 11 of the mixed differences: pair m / 4 of (x, y), (x, z), (y, z), corner m % 4 of ++, +-, -+, --; the first axis
// of the pair is moved by +-eps, then the second (this kernel's alone: no other probe takes a second difference)
__device__ __forceinline__ P3 mixed_point(int m, double eps, double px, double py, double pz) {
    const double ha = (m & 2) ? -eps : eps, hb = (m & 1) ? -eps : eps;
    P3 p = {px, py, pz};
    if ((m >> 2) == 0) { p.x = p.x + ha; p.y = p.y + hb; }
    else if ((m >> 2) == 1) { p.x = p.x + ha; p.z = p.z + hb; }
    else { p.y = p.y + ha; p.z = p.z + hb; }
    return p;
}

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < (double)INFINITY; }       // (false for NaN)

// g^T M g of a symmetric M in the definition's order
__device__ __forceinline__ double quad_form(double gx, double gy, double gz, double mxx, double myy, double mzz, double mxy, double mxz, double myz) {
    return ((gx * gx * mxx + gy * gy * myy) + gz * gz * mzz) + 2.0 * ((gx * gy * mxy + gx * gz * mxz) + gy * gz * myz);
}

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_vertex_curvature(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                          const double *__restrict__ pts, long long n, double eps,
                                                          double *__restrict__ out4, uint8_t *__restrict__ status_out,
                                                          unsigned long long *__restrict__ counts3) {
    const long long wave0 = (long long)blockIdx.x * 256 + (long long)(threadIdx.x & ~63u);
    if (wave0 >= n) return;                                            // (wave-uniform)
    const long long i = wave0 + (long long)(threadIdx.x & 63u);
    const bool live = i < n;
    const long long j = live ? i : n - 1;
    const double px = pts[3 * j], py = pts[3 * j + 1], pz = pts[3 * j + 2];
    const double two_eps = 2.0 * eps, eps2 = eps * eps, four_eps2 = (4.0 * eps) * eps;
    double v0 = 0.0, gx = 0.0, gy = 0.0, gz = 0.0, hxx = 0.0, hyy = 0.0, hzz = 0.0, hxy = 0.0, hxz = 0.0, hyz = 0.0;
    double ta = 0.0, tb = 0.0;                                         // the two temporaries of a difference in progress
    bool bad = false;                                                  // one of the 19 values is not finite
#pragma unroll 1
    for (int k = 0; k < 19; k++) {                                     // (k is wave-uniform, like every condition on it below)
        P3 p = {px, py, pz};
        if (k >= 7) p = mixed_point(k - 7, eps, px, py, pz);
        else if (k >= 1) p = grad_point(k - 1, eps, px, py, pz);
        const double v = (double)run_tape1<T, FULL>(code, consts, (T)p.x, (T)p.y, (T)p.z);
        bad = bad | !finite64(v);
        if (k == 0) {
            v0 = v;
        } else if (k < 7) {
            if ((k - 1) & 1) {                                         // the minus side: G_a and H_aa are complete
                const double g = (ta - v) / two_eps, h = (tb + (v - v0)) / eps2;
                if (k == 2) { gx = g; hxx = h; }
                else if (k == 4) { gy = g; hyy = h; }
                else { gz = g; hzz = h; }
            } else {
                ta = v; tb = v - v0;
            }
        } else {
            const int c = (k - 7) & 3;
            if (c == 1) {
                tb = ta - v;                                           // v++ - v+-
            } else if (c == 3) {
                const double h = (tb - (ta - v)) / four_eps2;          // ... - (v-+ - v--)
                if (k == 10) hxy = h;
                else if (k == 14) hxz = h;
                else hyz = h;
            } else {
                ta = v;
            }
        }
    }
    const double l2 = grad_len2(gx, gy, gz);
    const double l = sqrt(l2);
    const double tr = (hxx + hyy) + hzz;
    const double ghg = quad_form(gx, gy, gz, hxx, hyy, hzz, hxy, hxz, hyz);
    const double mean = (l2 * tr - ghg) / ((2.0 * l2) * l);
    const double axx = hyy * hzz - hyz * hyz, ayy = hxx * hzz - hxz * hxz, azz = hxx * hyy - hxy * hxy;
    const double axy = hxz * hyz - hxy * hzz, axz = hxy * hyz - hxz * hyy, ayz = hxy * hxz - hxx * hyz;
    const double gauss = quad_form(gx, gy, gz, axx, ayy, azz, axy, axz, ayz) / (l2 * l2);
    const double d = mean * mean - gauss;
    const double s = sqrt(d > 0.0 ? d : 0.0);
    const double k1 = mean + s, k2 = mean - s;
    const bool flat = l2 == 0.0 || !finite64(l);
    const bool broken = !(finite64(mean) && finite64(gauss) && finite64(k1) && finite64(k2));
    const int status = bad ? C_NAN : (flat ? C_FLAT : (broken ? C_NAN : C_CURVED));
    const unsigned long long curved_lanes = __ballot(live && status == C_CURVED), flat_lanes = __ballot(live && status == C_FLAT),
                             nan_lanes = __ballot(live && status == C_NAN);
    if (live) {
        const double none = __longlong_as_double(0x7ff8000000000000ll);        // np.nan's bits, by a select: never an arithmetic NaN
        const bool ok = status == C_CURVED;
        out4[4 * i] = ok ? mean : none;
        out4[4 * i + 1] = ok ? gauss : none;
        out4[4 * i + 2] = ok ? k1 : none;
        out4[4 * i + 3] = ok ? k2 : none;
        status_out[i] = (uint8_t)status;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (curved_lanes != 0ull) atomicAdd(counts3 + C_CURVED, (unsigned long long)__popcll(curved_lanes));
        if (flat_lanes != 0ull) atomicAdd(counts3 + C_FLAT, (unsigned long long)__popcll(flat_lanes));
        if (nan_lanes != 0ull) atomicAdd(counts3 + C_NAN, (unsigned long long)__popcll(nan_lanes));
    }
}

namespace sdfk {

// enqueue only: the curvatures of n >= 1 vertices (n x 3 float64 at d_pts) into d_out4 (n x 4: mean, gauss, k1, k2) and d_status, the
// number of vertices of each status added to d_counts3 (the caller has zeroed it on `st`).  Returns a hipError_t value (0 = ok).
int launch_vertex_curvature(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                            double eps, double *d_out4, uint8_t *d_status, unsigned long long *d_counts3) {
    if (n < 1) return 0;
    const unsigned grid = (unsigned)((n + 255) / 256);                 // (n < 2^31 vertices: the weld's limit)
    LAUNCH_F64_ON(st, k_vertex_curvature, dim3(grid), dim3(256), 0, full, d_code, d_consts, d_pts, n, eps, d_out4, d_status, d_counts3);
    return (int)hipGetLastError();
}

}  // namespace sdfk
