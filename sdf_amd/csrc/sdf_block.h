// sdf_block.h -- what the plain kernels of the mesh readers share on the DEVICE: the keys of a bounding box, a workgroup's integer
// sums added with one atomic, the halving tree over 256 float64 accumulators, a box reduced across the workgroup.  The host tools of
// the same units are in sdf_runtime.h and sdf_prims.h.
//
// FOR UNITS OF FLAG CLASS `plain` ONLY (build.units).  These helpers hold barriers and cross-lane moves; a unit built with the
// interpreters' structurizer option must not include this header (sdf_normals.hip keeps its own ballot).
//
// Every workgroup here is 256 lanes, four waves of 64.  A helper that holds a barrier is called by EVERY lane of the workgroup: no
// lane may have returned before the call, and the call stands under no condition that lanes of one workgroup answer differently.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfk {

// ---- the keys of a bounding box that integer atomics can take: float64 -> u64 whose unsigned order is the float order; both
// zeros give the key of +0.0 ----
__device__ __forceinline__ unsigned long long box_key(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__host__ __device__ __forceinline__ unsigned long long box_bits(unsigned long long k) { return (k >> 63) ? (k & ~(1ull << 63)) : ~k; }
// a key back to its double, on either side
__host__ __device__ __forceinline__ double box_value(unsigned long long k) {
    const unsigned long long u = box_bits(k);
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}
// the empty box: every lower bound is the key of +inf, every upper bound the key of -inf
constexpr unsigned long long BOX_EMPTY_LO = 0xfff0000000000000ull, BOX_EMPTY_HI = ~BOX_EMPTY_LO;

__device__ __forceinline__ bool finite9(const double *v) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && __builtin_isfinite(v[k]);
    return ok;
}

// ---- integer sums.  Every lane counts in registers; the lanes of a wave, then the four waves, are added up and ONE integer atomic
// per workgroup and counter that has any goes out (k_edge_classes measured one per wave and key tile first: 138,000 atomics on one
// cache line, 1.4 - 2.7 ms).  Integer sums do not depend on their order. ----
template <typename V>
__device__ __forceinline__ V wave_sum(V v) {                           // (lane 0 of the wave ends with the sum)
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_down(v, h);
    return v;
}
__device__ __forceinline__ unsigned wave_count(bool p) { return (unsigned)__popcll(__ballot(p)); }

// counter c of the workgroup is the sum of w[c] over the lanes 0 of its four waves: total[c] += it.  LDS of its own and ONE barrier,
// so a kernel calls it once, with all N of its counters (a second call would write the LDS that lanes of the first may still read);
// lanes < N issue at most one atomic each, and none for a sum of zero.  V holds a wave's sum, T the workgroup's.
template <int N, typename V, typename T>
__device__ __forceinline__ void block_add_waves(const V (&w)[N], T *total) {
    __shared__ V w_v[N][4];
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int c = 0; c < N; c++) w_v[c][threadIdx.x >> 6] = w[c];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const T sum = (T)w_v[threadIdx.x][0] + w_v[threadIdx.x][1] + w_v[threadIdx.x][2] + w_v[threadIdx.x][3];
        if (sum) atomicAdd(total + threadIdx.x, sum);
    }
}
// total[c] += the workgroup's sum of v[c]: every lane passes its own N values ...
template <int N, typename V, typename T>
__device__ __forceinline__ void block_add(const V (&v)[N], T *total) {
    V w[N];
#pragma unroll
    for (int c = 0; c < N; c++) w[c] = wave_sum(v[c]);
    block_add_waves(w, total);
}
// ... or its N flags
template <int N, typename T>
__device__ __forceinline__ void block_count(const bool (&p)[N], T *total) {
    unsigned w[N];
#pragma unroll
    for (int c = 0; c < N; c++) w[c] = wave_count(p[c]);
    block_add_waves(w, total);
}
// where a kernel has no barrier and is to gain none: one atomic per WAVE that has any (n: the wave's count, the same in its lanes)
template <typename T>
__device__ __forceinline__ void wave_add(unsigned n, T *total) {
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(total, (T)n);
}

// ---- the halving tree over the 256 lanes' float64 accumulators: x[:h] + x[h:], h = 128 ... 1 -- through LDS across the waves
// (h = 128, 64), by cross-lane moves inside wave 0 (h = 32 ... 1); lane 0 ends with the sums.  `tile`: >= 128 x SUMS doubles of LDS
// that no lane still reads.  tests/measure_ref.py, overhang_ref.py and supports_ref.py fix this order. ----
template <int SUMS>
__device__ __forceinline__ void tree256(double *acc, double *tile) {
    const int tid = (int)threadIdx.x;
    for (int h = 128; h >= 64; h >>= 1) {
        if (tid >= h && tid < 2 * h) {
#pragma unroll
            for (int k = 0; k < SUMS; k++) tile[k * 128 + (tid - h)] = acc[k];
        }
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < SUMS; k++) acc[k] = acc[k] + tile[k * 128 + tid];
        }
        __syncthreads();
    }
    if (tid < 64) {                                                    // (wave 0, whole)
        for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
            for (int k = 0; k < SUMS; k++) acc[k] = acc[k] + __shfl_down(acc[k], h);
        }
    }
}

// ---- a box on ordered keys K (box_key's u64, or plain int indices): lo[3] min, hi[3] max.  A lane that holds nothing holds the
// identities (the largest K in lo, the smallest in hi). ----
template <typename K>
__device__ __forceinline__ void wave_box_min_max(K (&lo)[3], K (&hi)[3]) {                 // (lane 0 of the wave ends with the wave's box)
    for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const K a = __shfl_down(lo[c], h), b = __shfl_down(hi[c], h);
            lo[c] = a < lo[c] ? a : lo[c];
            hi[c] = b > hi[c] ? b : hi[c];
        }
    }
}
// box[0..2] min, box[3..5] max take in the boxes that the lanes 0 of the four waves hold.  The waves meet in LDS (of its own, ONE
// barrier: once per kernel); six lanes take one bound each and touch the box only where they improve it (a stale read of the box
// can only ask for an atomic that was not needed): a handful of integer atomics per launch, not six per wave -- and none for the
// identities, if the box started no wider than empty
template <typename K>
__device__ __forceinline__ void block_box_merge(const K (&lo)[3], const K (&hi)[3], K *box) {
    __shared__ K wave_box[4][6];
    const int tid = (int)threadIdx.x;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { wave_box[tid >> 6][c] = lo[c]; wave_box[tid >> 6][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (tid < 6) {
        K v = wave_box[0][tid];
        for (int w = 1; w < 4; w++) {
            const K x = wave_box[w][tid];
            v = tid < 3 ? (x < v ? x : v) : (x > v ? x : v);
        }
        const K now = __atomic_load_n(box + tid, __ATOMIC_RELAXED);
        if (tid < 3) { if (v < now) atomicMin(box + tid, v); }
        else if (v > now) atomicMax(box + tid, v);
    }
}

}  // namespace sdfk
