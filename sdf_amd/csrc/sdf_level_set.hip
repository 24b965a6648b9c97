// sdf_level_set.hip -- triangle mesh -> dense narrow-band signed-distance grid on the device (sdf_mesh_level_set_host).
//
// What the reference gets from OpenVDB's createLevelSetFromPolygons + copyToArray (reference sdf/mesh.py:64-113), defined
// exactly so that tests/level_set_ref.py restates it bit for bit:
//   * voxel (i, j, k) sits at (i*vs, j*vs, k*vs), float64;
//   * d = sqrt(min over triangles of the squared point-triangle distance), Ericson's closest-point region test (Real-Time
//     Collision Detection 5.1.5) in one fixed operation order; degenerate triangles give the minimum over their edges;
//   * inside iff an odd number of triangles cross the voxel's +z column strictly below it: a watertight crossing test
//     (canonical edge functions, symbolic perturbation of the query point for E == 0);
//   * v = float32(min(d, background)), negated inside (a distance of 0 stays +0.0);
//   * the returned array is the index box of the voxels with |v| < background.
//
// Phases, all on the caller's stream, in ONE device allocation that is freed before the call returns:
//   k_ls_dist     one wave per triangle: every voxel of its band-expanded bounding box gets the float64 squared distance,
//                 kept as the minimum by atomicMin on the bit pattern (non-negative doubles order like their bits)
//   k_ls_sign     one wave per triangle: every column of its xy bounding box it covers flips bit k0 of that column's mask
//                 (atomicXor: the order of the flips does not matter)
//   k_ls_parity   one thread per column: prefix XOR along k -> the inside bit of every voxel
//   k_ls_compose  one thread per voxel: v, plus the index box of the active voxels (the box reduction of sdf_block.h)
//   k_ls_crop     the active box, packed for the copy to the host
// Built with -ffp-contract=off (csrc/build.sh): every multiply and add rounds separately, as NumPy's do.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "sdf_block.h"
#include "sdf_internal.h"

namespace sdfk {

struct LsGrid {
    long long lo[3];   // global voxel index of work voxel (0, 0, 0)
    int n[3];          // work grid dims
    int nw;            // 32-bit mask words per column
    double vs;         // voxel size
    double reach;      // a triangle farther than this from a voxel cannot change its value (background + margin)
    double skip_d2;    // squared distances above this are background anyway: not written
    float bg;          // background (float32(half_width_voxels * vs))
};

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 axpy(V3 a, V3 d, double t) { return {a.x + d.x * t, a.y + d.y * t, a.z + d.z * t}; }   // a + d * t
__device__ __forceinline__ double dist2(V3 p, V3 q) { const V3 e = sub(p, q); return dot(e, e); }

// squared distance from p to the segment a-b: t = clamp(dot(p - a, b - a) / dot(b - a, b - a), 0, 1)
__device__ __forceinline__ double seg_d2(V3 p, V3 a, V3 b) {
    const V3 ab = sub(b, a);
    const double l = dot(ab, ab);
    if (l == 0.0) return dist2(p, a);
    double t = dot(sub(p, a), ab) / l;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    return dist2(p, axpy(a, ab, t));
}

__device__ __forceinline__ double edges_d2(V3 p, V3 a, V3 b, V3 c) {
    return fmin(fmin(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a));
}

// Ericson 5.1.5 (ClosestPtPointTriangle), squared distance; a zero region denominator falls back to the edges
__device__ __forceinline__ double tri_d2(V3 p, V3 a, V3 b, V3 c, bool degen) {
    if (degen) return edges_d2(p, a, b, c);
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return dist2(p, a);
    const V3 bp = sub(p, b);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return dist2(p, b);
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double den = d1 - d3;
        if (den == 0.0) return edges_d2(p, a, b, c);
        return dist2(p, axpy(a, ab, d1 / den));
    }
    const V3 cp = sub(p, c);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return dist2(p, c);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double den = d2 - d6;
        if (den == 0.0) return edges_d2(p, a, b, c);
        return dist2(p, axpy(a, ac, d2 / den));
    }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
        const double den = e43 + e56;
        if (den == 0.0) return edges_d2(p, a, b, c);
        return dist2(p, axpy(b, sub(c, b), e43 / den));
    }
    const double den = va + vb + vc;
    if (den == 0.0) return edges_d2(p, a, b, c);
    const double inv = 1.0 / den;
    const double v = vb * inv, w = vc * inv;
    return dist2(p, axpy(axpy(a, ab, v), ac, w));
}

__device__ __forceinline__ void load_tri(const double *pts, const int *tris, long long t, V3 v[3]) {
    for (int e = 0; e < 3; e++) {
        const long long q = 3ll * tris[3 * t + e];
        v[e] = {pts[q], pts[q + 1], pts[q + 2]};
    }
}

// [first, last] global indices of the voxels whose coordinate can lie in [lo, hi], clamped to the work grid
__device__ __forceinline__ bool index_range(double lo, double hi, double vs, long long g0, int n, long long &a, long long &b) {
    a = (long long)floor(lo / vs) - g0;
    b = (long long)ceil(hi / vs) - g0;
    if (a < 0) a = 0;
    if (b > n - 1) b = n - 1;
    return a <= b;
}

// the voxels s = lane, lane + 64, ... of the box r0 + [0, ni) x [0, nj) x [0, nk) (k fastest: the lanes of a wave write adjacent voxels)
template <typename I>
__device__ __forceinline__ void dist_box(const V3 v[3], bool degen, const long long r0[3], I nj, I nk, I cnt, int lane, const LsGrid &g,
                                         unsigned long long *__restrict__ d2) {
    for (I s = lane; s < cnt; s += 64) {
        const I ij = s / nk;
        const long long k = r0[2] + (long long)(s - ij * nk), i = r0[0] + (long long)(ij / nj), j = r0[1] + (long long)(ij % nj);
        const V3 p = {(double)(g.lo[0] + i) * g.vs, (double)(g.lo[1] + j) * g.vs, (double)(g.lo[2] + k) * g.vs};
        const double q = tri_d2(p, v[0], v[1], v[2], degen);
        if (!(q <= g.skip_d2)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(q);
        unsigned long long *dst = d2 + ((unsigned long long)i * g.n[1] + j) * g.n[2] + k;
        // (a stale read only costs an atomic that changes nothing: the stored value never grows)
        if (bits < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, bits);
    }
}

// one wave per triangle (four per workgroup); every voxel of the triangle's bounding box grown by `reach`
__global__ __launch_bounds__(256) void k_ls_dist(const double *__restrict__ pts, const int *__restrict__ tris, long long nt, LsGrid g,
                                                 unsigned long long *__restrict__ d2) {
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= nt) return;
    V3 v[3];
    load_tri(pts, tris, t, v);
    const V3 ab = sub(v[1], v[0]), ac = sub(v[2], v[0]);
    const bool degen = ab.y * ac.z - ab.z * ac.y == 0.0 && ab.z * ac.x - ab.x * ac.z == 0.0 && ab.x * ac.y - ab.y * ac.x == 0.0;
    long long r0[3], r1[3];
    const double *c0 = &v[0].x, *c1 = &v[1].x, *c2 = &v[2].x;
    for (int a = 0; a < 3; a++) {
        const double mn = fmin(fmin(c0[a], c1[a]), c2[a]), mx = fmax(fmax(c0[a], c1[a]), c2[a]);
        if (!index_range(mn - g.reach, mx + g.reach, g.vs, g.lo[a], g.n[a], r0[a], r1[a])) return;
    }
    const long long ni = r1[0] - r0[0] + 1, nj = r1[1] - r0[1] + 1, nk = r1[2] - r0[2] + 1;
    const long long cnt = ni * nj * nk;
    if (cnt < 0xffffffffll) dist_box<unsigned>(v, degen, r0, (unsigned)nj, (unsigned)nk, (unsigned)cnt, lane, g, d2);   // (32-bit index arithmetic)
    else dist_box<unsigned long long>(v, degen, r0, nj, nk, cnt, lane, g, d2);
}

// the resolved sign of the projected edge function of edge P -> Q at q, and its value (canonical endpoints: the
// lexicographically smaller one is a; the other direction negates both)
__device__ __forceinline__ int edge_sign(double px, double py, double qx, double qy, double x, double y, double &E) {
    const bool fwd = px < qx || (px == qx && py < qy);
    const double ax = fwd ? px : qx, ay = fwd ? py : qy, bx = fwd ? qx : px, by = fwd ? qy : py;
    const double dx = bx - ax, dy = by - ay;
    const double e = dx * (y - ay) - dy * (x - ax);
    int s = e > 0.0 ? 1 : (e < 0.0 ? -1 : (-dy > 0.0 ? 1 : (-dy < 0.0 ? -1 : (dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0)))));
    E = fwd ? e : -e;
    return fwd ? s : -s;
}

// one wave per triangle: the columns of its xy bounding box it covers flip bit k0 of their mask
__global__ __launch_bounds__(256) void k_ls_sign(const double *__restrict__ pts, const int *__restrict__ tris, long long nt, LsGrid g,
                                                 unsigned *__restrict__ mask) {
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= nt) return;
    V3 v[3];
    load_tri(pts, tris, t, v);
    long long r0[2], r1[2];
    const double *c0 = &v[0].x, *c1 = &v[1].x, *c2 = &v[2].x;
    for (int a = 0; a < 2; a++) {
        const double mn = fmin(fmin(c0[a], c1[a]), c2[a]), mx = fmax(fmax(c0[a], c1[a]), c2[a]);
        if (!index_range(mn, mx, g.vs, g.lo[a], g.n[a], r0[a], r1[a])) return;
    }
    const long long nj = r1[1] - r0[1] + 1, cnt = (r1[0] - r0[0] + 1) * nj;
    for (long long s = lane; s < cnt; s += 64) {
        const long long i = r0[0] + s / nj, j = r0[1] + s % nj;
        const double x = (double)(g.lo[0] + i) * g.vs, y = (double)(g.lo[1] + j) * g.vs;
        double E0, E1, E2;
        const int s0 = edge_sign(v[1].x, v[1].y, v[2].x, v[2].y, x, y, E0);
        const int s1 = edge_sign(v[2].x, v[2].y, v[0].x, v[0].y, x, y, E1);
        const int s2 = edge_sign(v[0].x, v[0].y, v[1].x, v[1].y, x, y, E2);
        if (s0 == 0 || s0 != s1 || s0 != s2) continue;
        const double sum = E0 + E1 + E2;
        const double zc = sum == 0.0 ? v[0].z : (E0 * v[0].z + E1 * v[1].z + E2 * v[2].z) / sum;
        // k0: the smallest k with k * vs > zc, decided on the products themselves
        double k = floor(zc / g.vs) - 2.0;
        for (int r = 0; r < 5; r++) if (k * g.vs <= zc) k += 1.0;
        long long kw = (long long)k - g.lo[2];
        if (kw >= g.n[2]) continue;
        if (kw < 0) kw = 0;
        atomicXor(mask + ((unsigned long long)i * g.n[1] + j) * g.nw + (kw >> 5), 1u << (kw & 31));
    }
}

// one thread per column: prefix XOR of the flips along k (bit k of word k/32 = the voxel is inside)
__global__ __launch_bounds__(256) void k_ls_parity(unsigned *__restrict__ mask, long long ncol, int nw) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncol) return;
    unsigned carry = 0;
    for (int w = 0; w < nw; w++) {
        unsigned x = mask[c * nw + w];
        x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
        x ^= carry;
        mask[c * nw + w] = x;
        carry = (x >> 31) ? 0xffffffffu : 0u;
    }
}

// one thread per voxel (grid-stride): the value, and the index box of the voxels with |v| < background
// (box: min i, j, k then max i, j, k in work indices)
__global__ __launch_bounds__(256) void k_ls_compose(const unsigned long long *__restrict__ d2, const unsigned *__restrict__ mask, LsGrid g,
                                                    float *__restrict__ val, int *__restrict__ box) {
    const long long n = (long long)g.n[0] * g.n[1] * g.n[2];
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-1, -1, -1};
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n; s += (long long)gridDim.x * 256) {
        const unsigned long long bits = d2[s];
        const double d = bits > 0x7ff0000000000000ull ? (double)INFINITY : sqrt(__longlong_as_double((long long)bits));
        const double bg = (double)g.bg;
        float v = (float)(d < bg ? d : bg);
        const long long k = s % g.n[2], col = s / g.n[2];
        const bool inside = (mask[col * g.nw + (k >> 5)] >> (k & 31)) & 1u;
        if (inside && d != 0.0) v = -v;
        val[s] = v;
        if (fabsf(v) < g.bg) {
            const int c[3] = {(int)(col / g.n[1]), (int)(col % g.n[1]), (int)k};
            for (int a = 0; a < 3; a++) { mn[a] = min(mn[a], c[a]); mx[a] = max(mx[a], c[a]); }
        }
    }
    wave_box_min_max(mn, mx);                                          // (sdf_block.h, on int keys; the host starts the box at these identities)
    block_box_merge(mn, mx, box);
}

// the active box [c0, c0 + dims) of the work grid, packed [i][j][k]
__global__ __launch_bounds__(256) void k_ls_crop(const float *__restrict__ val, LsGrid g, int c0, int c1, int c2, int m1, int m2, long long m,
                                                 float *__restrict__ out) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const long long k = s % m2, ij = s / m2;
    const long long j = ij % m1, i = ij / m1;
    out[s] = val[((unsigned long long)(c0 + i) * g.n[1] + (c1 + j)) * g.n[2] + (c2 + k)];
}

static int refuse(const std::string &why) { fail("sdf_mesh_level_set_host: " + why); return 2; }

// the work grid of a validated mesh (all points finite, vs > 0): floor(min / vs) - hw - 1 .. ceil(max / vs) + hw + 1 per axis;
// refuses (2, with a message) a grid that cannot be indexed
static int plan(const double *pts, long long np, double vs, int hw, LsGrid &g) {
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long p = 0; p < np; p++)
        for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], pts[3 * p + a]); mx[a] = std::max(mx[a], pts[3 * p + a]); }
    double nvox = 1.0;
    for (int a = 0; a < 3; a++) {
        const double lo = floor(mn[a] / vs) - hw - 1, hi = ceil(mx[a] / vs) + hw + 1;
        if (!(fabs(lo) < 4.5e15 && fabs(hi) < 4.5e15) || hi - lo + 1 > 2147483647.0)
            return refuse("work grid axis " + std::to_string(a) + " spans " + std::to_string(hi - lo + 1) + " voxels: voxel size too small for this mesh");
        g.lo[a] = (long long)lo;
        g.n[a] = (int)(hi - lo + 1);
        nvox *= hi - lo + 1;
    }
    if (nvox > 4.0e12) return refuse("work grid of " + std::to_string(nvox) + " voxels: voxel size too small for this mesh");
    g.nw = (g.n[2] + 31) / 32;
    g.vs = vs;
    g.bg = (float)(hw * vs);
    // (a triangle whose bounding box is farther than the background from a voxel is farther than the background itself;
    // the margin only adds voxels whose result is the background anyway)
    g.reach = (double)g.bg * (1.0 + 1e-9) + vs * 1e-9;
    g.skip_d2 = (double)g.bg * (double)g.bg * (1.0 + 1e-9);
    return 0;
}

}  // namespace sdfk

using namespace sdfk;

// 0: done (dims reported; h_out filled when it holds them), 1: HIP error, 2: invalid arguments (nothing uploaded); sdf_last_error says why
extern "C" int sdf_mesh_level_set_host(sdf_ctx *c, const double *h_pts, int64_t np, const int32_t *h_tris, int64_t nt, double vs, int hw,
                                       int64_t out_ijk0[3], int64_t out_dims[3], float *h_out, int64_t cap) {
    if (!c || !out_ijk0 || !out_dims) return fail("sdf_mesh_level_set_host: NULL argument");
    HIPCHK(set_device(c->device));
    hipStream_t st = c->stream;
    for (int a = 0; a < 3; a++) { out_ijk0[a] = 0; out_dims[a] = 0; }
    if (np <= 0 || nt <= 0 || !h_pts || !h_tris) return refuse("empty mesh: no points or no triangles");
    if (!(vs > 0.0) || !std::isfinite(vs)) return refuse("voxel size must be a positive finite number");
    if (hw < 1 || hw > (1 << 20)) return refuse("half width must be 1 .. 2^20 voxels");
    if (np > (1ll << 31) || nt > (1ll << 31) / 3) return refuse("mesh too large for 32-bit indices");
    for (long long i = 0; i < 3 * np; i++)
        if (!std::isfinite(h_pts[i])) return refuse("point " + std::to_string(i / 3) + " is not finite");
    for (long long i = 0; i < 3 * nt; i++)
        if (h_tris[i] < 0 || h_tris[i] >= np)
            return refuse("triangle " + std::to_string(i / 3) + " indexes point " + std::to_string(h_tris[i]) + " of " + std::to_string((long long)np));
    LsGrid g = {};
    if (plan(h_pts, np, vs, hw, g)) return 2;
    const size_t n = (size_t)g.n[0] * g.n[1] * g.n[2], ncol = (size_t)g.n[0] * g.n[1];
    unsigned long long *d2;
    float *val;
    unsigned *mask;
    double *pts;
    int *tris, *dbox;
    Scratch scratch(st);
    scratch.part(&d2, n); scratch.part(&val, n); scratch.part(&mask, ncol * g.nw);
    scratch.part(&pts, (size_t)np * 3); scratch.part(&tris, (size_t)nt * 3); scratch.part(&dbox, 6);
    size_t free_b = 0;
    bool fits = false;
    HIPCHK_FN(mem_fits(scratch.bytes, &fits, &free_b));
    if (!fits)
        return refuse("work grid " + std::to_string(g.n[0]) + " x " + std::to_string(g.n[1]) + " x " + std::to_string(g.n[2]) + " needs " +
                      std::to_string(scratch.bytes) + " bytes of device memory, " + std::to_string(free_b) + " are free");
    const int box_init[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};
    int box[6] = {};
    const unsigned tri_blocks = (unsigned)((nt + 3) / 4);
    HIPCHK_FN(scratch.alloc());
    HIPCHK_FN(hipMemcpyAsync(pts, h_pts, (size_t)np * 24, hipMemcpyHostToDevice, st));
    HIPCHK_FN(hipMemcpyAsync(tris, h_tris, (size_t)nt * 12, hipMemcpyHostToDevice, st));
    HIPCHK_FN(hipMemcpyAsync(dbox, box_init, sizeof box_init, hipMemcpyHostToDevice, st));
    HIPCHK_FN(hipMemsetAsync(d2, 0xff, n * 8, st));            // (all ones: above every non-negative double -> no triangle in reach)
    HIPCHK_FN(hipMemsetAsync(mask, 0, ncol * g.nw * 4, st));
    HIPCHK_FN(launch_grid(k_ls_dist, tri_blocks, st, pts, tris, nt, g, d2));
    HIPCHK_FN(launch_grid(k_ls_sign, tri_blocks, st, pts, tris, nt, g, mask));
    HIPCHK_FN(launch_rows(k_ls_parity, (long long)ncol, st, mask, ncol, g.nw));
    HIPCHK_FN(launch_grid(k_ls_compose, (unsigned)std::min<size_t>((n + 255) / 256, 8192), st, d2, mask, g, val, dbox));
    HIPCHK_FN(hipMemcpyAsync(box, dbox, sizeof box, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(stream_wait(st));
    if (box[3] >= 0) {
        long long m = 1;
        for (int a = 0; a < 3; a++) {
            out_ijk0[a] = g.lo[a] + box[a];
            out_dims[a] = box[3 + a] - box[a] + 1;
            m *= out_dims[a];
        }
        if (h_out && m <= cap) {
            float *out = (float *)d2;                           // (the squared distances are consumed: the crop goes there)
            HIPCHK_FN(launch_rows(k_ls_crop, m, st, val, g, box[0], box[1], box[2], out_dims[1], out_dims[2], m, out));
            HIPCHK_FN(hipMemcpyAsync(h_out, out, (size_t)m * 4, hipMemcpyDeviceToHost, st));
            HIPCHK_FN(stream_wait(st));
        }
    }
    return 0;
}
