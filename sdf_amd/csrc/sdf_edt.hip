// sdf_edt.hip -- boolean mask -> signed exact Euclidean distance texture on the device (sdf_distance_texture_host).
//
// What `distance_texture` (sdf_amd/text.py; reference sdf/text.py:77-87) gets from two calls of scipy's distance_transform_edt,
// defined exactly so that tests/edt_ref.py restates it bit for bit.  For a mask `a` (rows x cols, one
// byte per pixel, non-zero = True) that holds both classes:
//   D(p)       = min over the pixels q with a[q] != a[p] of (p.row - q.row)^2 + (p.col - q.col)^2      (an integer >= 1)
//   texture[p] = -sqrt(double(D(p))) where a[p], +sqrt(double(D(p))) elsewhere                         (correctly rounded sqrt)
// All distance arithmetic is 32-bit integer: the host refuses masks with rows^2 + cols^2 >= 2^31.
//
// Separable, two kernels on the caller's stream, in ONE device allocation that is freed before the call returns.  The LONG axis
// (length L) is scanned, the SHORT one (length S) is searched, so that the search is bounded by S * S * L steps:
//   k_edt_scan   one workgroup per line along the long axis: the line becomes two bit masks in LDS (True / False, by __ballot);
//                a lane per pixel finds the nearest bit of the OTHER class before and after it (clz / ffs, walking words) and
//                writes g = +d for a True pixel, -d for a False one (d = EDT_NONE: the line holds no pixel of the other class)
//   k_edt_min    one workgroup per tile of TL neighbouring lines ACROSS the short axis, whose S * TL values of g are staged in LDS;
//                a lane per pixel i: D = min over j of h(j)^2 + (i - j)^2, h(j) = |g[j]| where pixel j has the class of pixel i
//                (its other-class distance along the line) and 0 where it is of the other class itself.  The search walks
//                j = i -+ k outwards and stops once k^2 >= the best value so far; then sqrt and sign, float64 out.
// Built with -ffp-contract=off like the rest (csrc/build.sh); the only floating-point operation is the final sqrt.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "sdf_internal.h"

namespace sdfk {

// "no pixel of the other class on this line": EDT_NONE^2 = 2147488281 >= 2^31 > every real D, and EDT_NONE^2 + k^2 (k < 16384)
// still fits 32 unsigned bits
#define EDT_NONE 46341
#define EDT_MAX_SHORT 16384      // S * TL ints of LDS, 64 KB at most: the short axis may not be longer
#define EDT_MAX_WORDS 725        // ceil(46340 / 64): words of one line's bit mask

// pixel (s, l) -- s along the short axis, l along the long one -- sits at s * stride_s + l * stride_l
struct EdtShape {
    int S, L;
    long long stride_s, stride_l;
};

__global__ __launch_bounds__(256) void k_edt_scan(const uint8_t *__restrict__ mask, EdtShape sh, int *__restrict__ g) {
    __shared__ unsigned long long bits[2][EDT_MAX_WORDS];     // [1]: the True pixels of the line, [0]: the False ones
    const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (sh.L + 63) >> 6;
    const long long base = (long long)s * sh.stride_s;
    for (int w = wave; w < nw; w += 4) {                       // (w is the same in every lane of a wave: the ballots are whole)
        const int l = w * 64 + lane;
        const bool in = l < sh.L;
        const bool t = in && mask[base + (long long)l * sh.stride_l] != 0;
        const unsigned long long bt = __ballot(t), bf = __ballot(in && !t);
        if (lane == 0) { bits[1][w] = bt; bits[0][w] = bf; }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < sh.L; l += 256) {
        const int w = l >> 6, b = l & 63;
        const int x = (int)((bits[1][w] >> b) & 1ull);
        const unsigned long long *m = bits[x ^ 1];             // the other class (its bit b of word w is clear)
        int d = EDT_NONE;
        unsigned long long mm = m[w] & (~0ull >> (63 - b));
        int ww = w;
        while (mm == 0 && ww > 0) mm = m[--ww];
        if (mm) d = l - (ww * 64 + 63 - __clzll((long long)mm));
        mm = m[w] & (~0ull << b);
        ww = w;
        while (mm == 0 && ww + 1 < nw) mm = m[++ww];
        if (mm) d = min(d, ww * 64 + __ffsll((unsigned long long)mm) - 1 - l);
        g[base + (long long)l * sh.stride_l] = x ? d : -d;
    }
}

// tl: lines per workgroup, a power of two (tl_log2 its logarithm); LDS: S * tl ints, [i][line]
__global__ __launch_bounds__(256) void k_edt_min(const int *__restrict__ g, EdtShape sh, int tl_log2, double *__restrict__ out) {
    extern __shared__ int v[];
    const int tl = 1 << tl_log2, l0 = blockIdx.x << tl_log2, n = sh.S << tl_log2;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int i = idx >> tl_log2, l = l0 + (idx & (tl - 1));
        v[idx] = l < sh.L ? g[(long long)i * sh.stride_s + (long long)l * sh.stride_l] : 0;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int i = idx >> tl_log2, l = l0 + (idx & (tl - 1));
        if (l >= sh.L) continue;
        const int own = v[idx];
        const int sgn = own > 0 ? 1 : -1;                      // h(j) = max(sgn * g[j], 0)
        unsigned h = (unsigned)(own * sgn);
        unsigned best = h * h;
        const int up = i, down = sh.S - 1 - i, far = max(up, down);
        unsigned kk = 1;
        // (four offsets per test of the bound: their eight LDS reads are in flight together; an offset past the bound is still a
        // real candidate, so the minimum is the same)
        for (int k = 1; k <= far && kk < best;) {
#pragma unroll
            for (int u = 0; u < 4; u++, kk += 2u * k + 1u, k++) {
                if (k <= up) {
                    h = (unsigned)max(v[idx - (k << tl_log2)] * sgn, 0);
                    best = min(best, h * h + kk);
                }
                if (k <= down) {
                    h = (unsigned)max(v[idx + (k << tl_log2)] * sgn, 0);
                    best = min(best, h * h + kk);
                }
            }
        }
        const double r = sqrt((double)best);
        out[(long long)i * sh.stride_s + (long long)l * sh.stride_l] = own > 0 ? -r : r;
    }
}

}  // namespace sdfk

using namespace sdfk;

// 0: done, 1: HIP error, 2: refused (nothing uploaded, nothing launched); sdf_last_error says why
extern "C" int sdf_distance_texture_host(sdf_ctx *c, const uint8_t *h_mask, int64_t rows, int64_t cols, double *h_out) {
    auto refuse = [](const std::string &why) { fail("sdf_distance_texture_host: " + why); return 2; };
    if (!c || !h_mask || !h_out) return refuse("NULL argument");
    HIPCHK(set_device(c->device));
    hipStream_t st = c->stream;
    const std::string shape = std::to_string(rows) + " x " + std::to_string(cols);
    if (rows < 1 || cols < 1) return refuse("empty mask: " + shape);
    // (either side above 46340 fails the first test by itself, so the squares below cannot overflow)
    if (rows > 46340 || cols > 46340 || rows * rows + cols * cols >= (1ll << 31))
        return refuse("mask of " + shape + ": rows^2 + cols^2 must stay below 2^31 (32-bit squared distances)");
    if (std::min(rows, cols) > EDT_MAX_SHORT)
        return refuse("mask of " + shape + ": the shorter side must not exceed " + std::to_string(EDT_MAX_SHORT) + " pixels (one line across it is kept in LDS)");
    const size_t n = (size_t)rows * (size_t)cols;
    {
        bool any_t = false, any_f = false;
        for (size_t p = 0; p < n && !(any_t && any_f); p++) {
            if (h_mask[p]) any_t = true;
            else any_f = true;
        }
        if (!(any_t && any_f))
            return refuse(std::string("every pixel of the mask is ") + (any_t ? "True" : "False") + ": the distance to the other class is undefined");
    }
    uint8_t *mask;
    int *g;
    double *out;
    Scratch scratch(st);
    scratch.part(&mask, n); scratch.part(&g, n); scratch.part(&out, n);
    size_t free_b = 0;
    bool fits = false;
    HIPCHK_FN(mem_fits(scratch.bytes, &fits, &free_b));
    if (!fits)
        return refuse("mask of " + shape + " needs " + std::to_string(scratch.bytes) + " bytes of device memory, " + std::to_string(free_b) + " are free");
    EdtShape sh;
    if (rows <= cols) { sh.S = (int)rows; sh.L = (int)cols; sh.stride_s = cols; sh.stride_l = 1; }
    else { sh.S = (int)cols; sh.L = (int)rows; sh.stride_s = 1; sh.stride_l = cols; }
    int tl_log2 = 4;                                           // 16 lines per workgroup while they fit 64 KB of LDS ...
    while (tl_log2 > 0 && ((size_t)sh.S << tl_log2) > EDT_MAX_SHORT) tl_log2--;
    // ... and down to 4 while that leaves fewer than 1024 workgroups: the search is a chain of dependent LDS reads, which only
    // several waves per SIMD hide
    while (tl_log2 > 2 && (sh.L >> tl_log2) < 1024) tl_log2--;
    const unsigned tiles = (unsigned)((sh.L + (1 << tl_log2) - 1) >> tl_log2);
    HIPCHK_FN(scratch.alloc());
    HIPCHK_FN(hipMemcpyAsync(mask, h_mask, n, hipMemcpyHostToDevice, st));
    HIPCHK_FN(launch_grid(k_edt_scan, (unsigned)sh.S, st, mask, sh, g));
    hipLaunchKernelGGL(k_edt_min, dim3(tiles), dim3(256), ((size_t)sh.S << tl_log2) * sizeof(int), st, (const int *)g, sh, tl_log2, out);
    HIPCHK_FN(hipGetLastError());
    HIPCHK_FN(hipMemcpyAsync(h_out, out, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(stream_wait(st));
    return 0;
}
