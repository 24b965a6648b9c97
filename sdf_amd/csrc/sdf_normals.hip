// sdf_normals.hip -- the field's gradient at the welded vertices of a mesh (sdf_mesh_vertex_normals, ABI 14): the
// vertex normals of the indexed PLY / OBJ export.  tests/normals_ref.py is the definition; this kernel reproduces it bit for bit over
// the interpreter that sdf_eval_points runs: float64, one rounding per written operation (-ffp-contract=off), for axis k the value at
// x_k + eps minus the value at x_k + (-eps), len = sqrt((g0*g0 + g1*g1) + g2*g2), n = g / len by division.  A vertex whose len is 0
// or NaN is FLAT: its normal is (0, 0, 0) and it is counted.
//
// A probe kernel (sdf_probe.h has the doctrine): one welded vertex per lane, one phase -- the six passes of the central difference.
// The flat vertices are counted by one integer atomic add per wave that has any.
#include "sdf_interp.h"
#include "sdf_normals.h"
#include "sdf_probe.h"

using namespace sdfk;

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_vertex_normals(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                        const double *__restrict__ pts, long long n, double eps,
                                                        double *__restrict__ out, unsigned long long *__restrict__ n_flat) {
    const long long wave0 = (long long)blockIdx.x * 256 + (long long)(threadIdx.x & ~63u);
    if (wave0 >= n) return;                                            // (wave-uniform)
    const long long i = wave0 + (long long)(threadIdx.x & 63u);
    const bool live = i < n;
    const long long j = live ? i : n - 1;
    const double px = pts[3 * j], py = pts[3 * j + 1], pz = pts[3 * j + 2];
    Grad g = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
        const P3 p = grad_point(k, eps, px, py, pz);
        const double v = (double)run_tape1<T, FULL>(code, consts, (T)p.x, (T)p.y, (T)p.z);
        g = grad_take(g, k, v);
    }
    const double len = sqrt(grad_len2(g.g0, g.g1, g.g2));
    const bool flat = grad_flat(len);
    const unsigned long long flat_lanes = __ballot(live && flat);
    if (live) {
        out[3 * i] = flat ? 0.0 : g.g0 / len;
        out[3 * i + 1] = flat ? 0.0 : g.g1 / len;
        out[3 * i + 2] = flat ? 0.0 : g.g2 / len;
    }
    if (flat_lanes != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(n_flat, (unsigned long long)__popcll(flat_lanes));
}

namespace sdfk {

// enqueue only: the normals of n >= 1 vertices (n x 3 float64 at d_pts) into d_out, the number of flat ones added to *d_flat
// (the caller has zeroed it on `st`).  Returns a hipError_t value (0 = ok).
int launch_vertex_normals(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_pts, long long n,
                          double eps, double *d_out, unsigned long long *d_flat) {
    if (n < 1) return 0;
    const unsigned grid = (unsigned)((n + 255) / 256);                 // (n < 2^31 vertices: the weld's limit)
    LAUNCH_F64_ON(st, k_vertex_normals, dim3(grid), dim3(256), 0, full, d_code, d_consts, d_pts, n, eps, d_out, d_flat);
    return (int)hipGetLastError();
}

}  // namespace sdfk
