// sdf_supports.hip -- support rays traced through the field (sdf_mesh_support_rays): from the centroid of every
// overhanging face of a mesh a ray is sphere-traced DOWNWARD, against the build direction, through the air until it meets the part or
// the bed plane; the bracket of a crossing is bisected and the ray's length is the height of the support column under the face.
// tests/supports_ref.py is the definition; this kernel reproduces it bit for bit over the interpreter that sdf_eval_points runs:
// float64, one rounding per written operation (-ffp-contract=off), dot = (x*x' + y*y') + z*z', a point on a ray is c + t * nd.
//
// A probe kernel (sdf_probe.h has the doctrine), k_vertex_thickness (sdf_thickness.hip) turned inside out: it marches while v >= 0
// and stops on v < 0.  One overhanging triangle per lane, in triangle order (d_triangle, numbered by the driver in sdf_overhang.hip),
// the phases MARCH -> REFINE: the march ends when `__any(status == MARCH)` says so or after max_steps passes, REFINE is skipped when
// no lane of the wave is PART, and a wave whose rays all begin at or below the bed evaluates nothing.  A lane that is done evaluates
// at its frozen parameter; a lane beyond the last ray repeats the last ray.
#include "sdf_interp.h"
#include "sdf_supports.h"

using namespace sdfk;

enum { S_BED = 0, S_PART = 1, S_BURIED = 2, S_UNRESOLVED = 3, S_NAN = 4, S_MARCH = 5 };      // (0 .. 4: the status codes of the ABI)
enum { PH_MARCH = 0, PH_REFINE = 1 };

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_support_rays(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                      const double *__restrict__ soup, const int32_t *__restrict__ triangle, long long m,
                                                      const SupportArgs a, double *__restrict__ height, uint8_t *__restrict__ status_out,
                                                      int32_t *__restrict__ steps_out, double *__restrict__ origin, double *__restrict__ terms) {
    const long long wave0 = (long long)blockIdx.x * 256 + (long long)(threadIdx.x & ~63u);
    if (wave0 >= m) return;                                            // (wave-uniform)
    const long long i = wave0 + (long long)(threadIdx.x & 63u);
    const bool live = i < m;
    const long long j = live ? i : m - 1;
    const double *p = soup + 9 * (long long)triangle[j];
    double v9[9];
#pragma unroll
    for (int c = 0; c < 9; c++) v9[c] = p[c];
    // n, dn as tests/overhang_ref.py writes them; the centroid and the distance to the bed as tests/supports_ref.py does
    const double ux = v9[3] - v9[0], uy = v9[4] - v9[1], uz = v9[5] - v9[2];
    const double wx = v9[6] - v9[0], wy = v9[7] - v9[1], wz = v9[8] - v9[2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double proj = -((nx * a.dx + ny * a.dy) + nz * a.dz);
    const double cx = ((v9[0] + v9[3]) + v9[6]) / 3.0, cy = ((v9[1] + v9[4]) + v9[7]) / 3.0, cz = ((v9[2] + v9[5]) + v9[8]) / 3.0;
    const double h = ((cx * a.dx + cy * a.dy) + cz * a.dz) - a.lo;
    const double tb = h > 0.0 ? h : 0.0;
    const double ndx = -a.dx, ndy = -a.dy, ndz = -a.dz;
    double t = a.start, lo = 0.0, hi = a.start;
    int status = a.start >= tb ? S_BED : S_MARCH, steps = 0;
    int phase = PH_MARCH, k = 0;                                       // (wave-uniform, like every condition on them below)
    if (__any(status == S_MARCH)) {
        for (;;) {
            // where this pass evaluates: the march's t, the bisection's midpoint
            const double mid = 0.5 * (lo + hi);
            const bool fix = status == S_PART;
            const double s = (phase == PH_REFINE && fix) ? mid : t;
            const double x = cx + s * ndx, y = cy + s * ndy, z = cz + s * ndz;
            const double v = (double)run_tape1<T, FULL>(code, consts, (T)x, (T)y, (T)z);
            if (phase == PH_MARCH) {
                const bool mch = status == S_MARCH;
                const bool nan = v != v, in = !nan && v < 0.0, go = !nan && !in;
                const double adv = v * a.step_scale;
                const double t1 = t + (adv > a.min_step ? adv : a.min_step);
                const bool down = t1 >= tb;
                steps += mch ? 1 : 0;
                hi = (mch && in) ? t : hi;
                lo = (mch && go) ? t : lo;
                status = !mch ? status : (nan ? S_NAN : (in ? (k == 0 ? S_BURIED : S_PART) : (down ? S_BED : S_MARCH)));
                t = (mch && go && !down) ? t1 : t;
                k++;
                if (!(__any(status == S_MARCH) && k < a.max_steps)) {
                    status = status == S_MARCH ? S_UNRESOLVED : status;    // ran out of steps
                    if (!(a.refine > 0 && __any(status == S_PART))) break;
                    phase = PH_REFINE; k = 0;
                }
            } else {
                const bool in = v < 0.0;
                hi = (fix && in) ? mid : hi;
                lo = (fix && !in) ? mid : lo;                          // (NaN included)
                k++;
                if (k == a.refine) break;
            }
        }
    }
    if (!live) return;
    const bool part = status == S_PART, buried = status == S_BURIED, bed = status == S_BED || status == S_UNRESOLVED;
    const double hgt = bed ? tb : (part ? hi : (buried ? 0.0 : __longlong_as_double(0x7ff8000000000000ll)));
    const double ph = proj * hgt;
    height[i] = hgt;
    status_out[i] = (uint8_t)status;
    steps_out[i] = steps;
    origin[3 * i] = cx; origin[3 * i + 1] = cy; origin[3 * i + 2] = cz;
    terms[i] = bed ? ph : 0.0;
    terms[m + i] = part ? ph : 0.0;
    terms[2 * m + i] = part ? proj : 0.0;
    terms[3 * m + i] = proj;
    terms[4 * m + i] = buried ? proj : 0.0;
}

namespace sdfk {

int launch_support_rays(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_soup,
                        const int32_t *d_triangle, long long m, const SupportArgs &a, double *d_height, uint8_t *d_status, int32_t *d_steps,
                        double *d_origin, double *d_terms) {
    if (m < 1) return 0;
    const unsigned grid = (unsigned)((m + 255) / 256);                 // (m < 2^31 triangles)
    LAUNCH_F64_ON(st, k_support_rays, dim3(grid), dim3(256), 0, full, d_code, d_consts, d_soup, d_triangle, m, a, d_height, d_status, d_steps,
                  d_origin, d_terms);
    return (int)hipGetLastError();
}

}  // namespace sdfk
