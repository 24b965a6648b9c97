// sdf_overhang.hip -- build directions rated where the mesh lies (sdf_mesh_overhangs, sdf_mesh_overhang_classes, added under ABI 17;
// DESIGN.md section 4n).  tests/overhang_ref.py is the definition; these kernels reproduce it bit for bit: float64, one rounding per
// written operation (-ffp-contract=off), and a summation TREE that depends on the order of the triangles and on nothing else.
//
// The work is dense, triangles x directions, and the lanes are the DIRECTIONS.  A workgroup of 256 lanes owns one chunk of
// OVERHANG_CHUNK = 1024 consecutive triangles and one group of 256 directions (four waves, 64 directions each); it walks the chunk in
// four tiles of 256 triangles.  Staging a tile: one triangle per lane -- the lane reads its nine coordinates and computes the raw
// normal n, dbl = |n| and the threshold -(sin_limit * dbl) once, 14 doubles into LDS (28 KB per tile).  A triangle that is not finite
// is staged with n and the threshold NaN: every comparison it meets is false, so it is neither overhang nor contact and adds +0.0.
// Walking a tile: the lanes change roles -- lane l holds direction l of its group and lo of that direction in registers and takes the
// staged triangles in index order; every LDS read is one address for the whole wave (a broadcast), nothing is reduced across lanes,
// and the three accumulators of a lane add the chunk's terms one after the other from +0.0: the definition's in-chunk order, for
// nothing.  Lanes beyond the last direction idle (one direction uses one lane in 256; profiles/overhang01_build_directions.md).
//
// Two passes.  k_overhang_extents: lo and hi of h(p) = (px dx + py dy) + pz dz per direction over the finite triangles, the same
// staging with the coordinates and a flag; the workgroups stride over the tiles and meet in 64-bit integer atomic min / max on
// box_key's keys (sdf_block.h) -- order-free and exact.  k_overhang_terms: the three terms and the two counts of a chunk, written
// as partials[direction][chunk][3] and one packed count word.  k_overhang_partials -- the shape of k_moment_partials, one partial
// per lane, the halving tree x[:h] + x[h:], h = 128 ... 1, spelt out in the kernel (a second copy of sdf_block.h's tree256, to be kept
// in step with it by hand: the kernel holds its parent's instructions that way, see the note there) -- takes 256 partials of one direction to one per launch until one is left
// (a single chunk goes through it once: x + 0.0 changes no bit of x >= +0.0); its first launch also adds up the packed counts,
// one integer atomic per workgroup and counter.  The directions go in slabs so that the partials stay under a cap; a slab changes which
// launch serves a direction and nothing a direction computes.
//
// k_overhang_classes: one direction, one triangle per lane, the same predicates, one byte per triangle.
//
// The support rays of section 4o (support_rays_run at the end of this file) take their faces from k_overhang_classes and their sums
// through k_overhang_partials; what they add here are plain kernels -- flags, numbering, the chunk walk, the status counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <string>
#include <vector>

#include "sdf_block.h"
#include "sdf_overhang.h"
#include "sdf_prims.h"
#include "sdf_runtime.h"
#include "sdf_supports.h"

namespace sdfk {

constexpr int OVERHANG_SUMS = 3;
constexpr int OVERHANG_TILE = 256;                 // triangles per tile = lanes per workgroup = directions per group
constexpr int OVERHANG_CHUNK = 1024;               // triangles per chunk (tests/overhang_ref.py: C)
constexpr int OVERHANG_STAGED = 14;                // a, b, c, n, dbl, threshold
constexpr int EXTENT_STAGED = 10;                  // a, b, c, finite (1.0 / 0.0)
// workgroups per direction group that stride over the tiles (k_overhang_extents).  A lane's min / max chain is serial, so with few
// directions the pass is bound by the length of a workgroup's walk: 512 workgroups with one chain per lane took 1.2 ms on 2.9 M
// triangles, most of a call with one direction (profiles/overhang01_build_directions.md); the atomics are two per lane and only
// where a bound improves
constexpr int EXTENT_MAX_BLOCKS = 1024;

// one lane per direction of the slab: the empty extents, no triangles counted
__global__ __launch_bounds__(256) void k_overhang_init(long long n_dirs, unsigned long long *__restrict__ ext, unsigned long long *__restrict__ counts) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < n_dirs) {
        ext[2 * k] = BOX_EMPTY_LO; ext[2 * k + 1] = BOX_EMPTY_HI;
        counts[2 * k] = 0ull; counts[2 * k + 1] = 0ull;
    }
}

// grid: striding workgroups x direction groups (the group varies fastest, so neighbours read the same triangles); ext[direction][lo, hi]
__global__ __launch_bounds__(256) void k_overhang_extents(const double *__restrict__ soup, long long n_tris, const double *__restrict__ dirs,
                                                          long long n_dirs, unsigned n_dgroups, unsigned long long *__restrict__ ext) {
    __shared__ __attribute__((aligned(16))) double tile[EXTENT_STAGED * OVERHANG_TILE];
    const int tid = (int)threadIdx.x;
    const long long k = (long long)(blockIdx.x % n_dgroups) * OVERHANG_TILE + tid;
    const bool active = k < n_dirs;
    const double dx = active ? dirs[3 * k] : 0.0, dy = active ? dirs[3 * k + 1] : 0.0, dz = active ? dirs[3 * k + 2] : 0.0;
    const long long n_tiles = (n_tris + OVERHANG_TILE - 1) / OVERHANG_TILE;
    const long long stride = (long long)(gridDim.x / n_dgroups);
    double lo = INFINITY, hi = -INFINITY, lo_b = INFINITY, hi_b = -INFINITY, lo_c = INFINITY, hi_c = -INFINITY;      // (a chain per vertex: min and max are order-free)
    for (long long tl = (long long)(blockIdx.x / n_dgroups); tl < n_tiles; tl += stride) {           // (uniform in the workgroup)
        const long long t0 = tl * OVERHANG_TILE;
        const int cnt = (int)(n_tris - t0 < OVERHANG_TILE ? n_tris - t0 : OVERHANG_TILE);
        __syncthreads();
        if (tid < cnt) {
            const double *src = soup + 9 * (t0 + tid);
            double *dst = tile + EXTENT_STAGED * tid;
            bool ok = true;                                            // (not finite9: through it the kernel's float64 instructions moved)
#pragma unroll
            for (int c = 0; c < 9; c++) { const double v = src[c]; ok = ok && __builtin_isfinite(v); dst[c] = v; }
            dst[9] = ok ? 1.0 : 0.0;
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < cnt; j++) {
                const double *v = tile + EXTENT_STAGED * j;
                if (v[9] != 0.0) {                                     // (uniform: every lane looks at triangle j)
                    const double ha = (v[0] * dx + v[1] * dy) + v[2] * dz;
                    const double hb = (v[3] * dx + v[4] * dy) + v[5] * dz;
                    const double hc = (v[6] * dx + v[7] * dy) + v[8] * dz;
                    lo = ha < lo ? ha : lo; lo_b = hb < lo_b ? hb : lo_b; lo_c = hc < lo_c ? hc : lo_c;
                    hi = ha > hi ? ha : hi; hi_b = hb > hi_b ? hb : hi_b; hi_c = hc > hi_c ? hc : hi_c;
                }
            }
        }
    }
    lo = lo_b < lo ? lo_b : lo; lo = lo_c < lo ? lo_c : lo;
    hi = hi_b > hi ? hi_b : hi; hi = hi_c > hi ? hi_c : hi;
    if (active && lo <= hi) {
        // a stale read of the extents can only ask for an atomic that was not needed
        const unsigned long long kl = box_key(lo), kh = box_key(hi);
        if (kl < __atomic_load_n(ext + 2 * k, __ATOMIC_RELAXED)) atomicMin(ext + 2 * k, kl);
        if (kh > __atomic_load_n(ext + 2 * k + 1, __ATOMIC_RELAXED)) atomicMax(ext + 2 * k + 1, kh);
    }
}

// the nine coordinates of a triangle -> n, dbl, finite; as tests/overhang_ref.py::triangle_parts writes them
__device__ __forceinline__ bool triangle_parts(const double *v, double *n, double *dbl) {
    bool ok = true;                                                    // (not finite9 behind the normal: that moved k_overhang_terms' float64 instructions)
#pragma unroll
    for (int c = 0; c < 9; c++) ok = ok && __builtin_isfinite(v[c]);
    const double ux = v[3] - v[0], uy = v[4] - v[1], uz = v[5] - v[2];
    const double wx = v[6] - v[0], wy = v[7] - v[1], wz = v[8] - v[2];
    n[0] = uy * wz - uz * wy; n[1] = uz * wx - ux * wz; n[2] = ux * wy - uy * wx;
    *dbl = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    return ok;
}

// grid: n_chunks x direction groups (the group varies fastest).  partials[direction][chunk][3]; packed[direction][chunk] =
// overhanging | bed-contact << 16 triangles of the chunk (each <= 1024)
__global__ __launch_bounds__(256) void k_overhang_terms(const double *__restrict__ soup, long long n_tris, const double *__restrict__ dirs,
                                                        long long n_dirs, unsigned n_dgroups, long long n_chunks,
                                                        const unsigned long long *__restrict__ ext, double sin_limit, double bed_tol,
                                                        double *__restrict__ partials, unsigned *__restrict__ packed) {
    __shared__ __attribute__((aligned(16))) double tile[OVERHANG_STAGED * OVERHANG_TILE];
    const int tid = (int)threadIdx.x;
    const long long chunk = (long long)(blockIdx.x / n_dgroups);
    const long long k = (long long)(blockIdx.x % n_dgroups) * OVERHANG_TILE + tid;
    const bool active = k < n_dirs;
    const double dx = active ? dirs[3 * k] : 0.0, dy = active ? dirs[3 * k + 1] : 0.0, dz = active ? dirs[3 * k + 2] : 0.0;
    const double lo = active ? box_value(ext[2 * k]) : 0.0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    unsigned n_over = 0u, n_contact = 0u;
    const long long c0 = chunk * OVERHANG_CHUNK;
#pragma unroll 1
    for (int s = 0; s < OVERHANG_CHUNK / OVERHANG_TILE; s++) {
        const long long t0 = c0 + (long long)s * OVERHANG_TILE;
        if (t0 >= n_tris) break;                                       // (uniform)
        const int cnt = (int)(n_tris - t0 < OVERHANG_TILE ? n_tris - t0 : OVERHANG_TILE);
        __syncthreads();
        if (tid < cnt) {
            const double *src = soup + 9 * (t0 + tid);
            double v[9], n[3], dbl;
#pragma unroll
            for (int c = 0; c < 9; c++) v[c] = src[c];
            const bool ok = triangle_parts(v, n, &dbl);
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            double *dst = tile + OVERHANG_STAGED * tid;
#pragma unroll
            for (int c = 0; c < 9; c++) dst[c] = v[c];
            dst[9] = ok ? n[0] : nan; dst[10] = ok ? n[1] : nan; dst[11] = ok ? n[2] : nan;
            dst[12] = dbl;
            dst[13] = ok ? -(sin_limit * dbl) : nan;
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < cnt; j++) {
                const double2 *q = reinterpret_cast<const double2 *>(tile + OVERHANG_STAGED * j);      // (112 bytes a triangle: 16-byte aligned)
                const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5], q6 = q[6];
                const double ha = ((q0.x * dx + q0.y * dy) + q1.x * dz) - lo;
                const double hb = ((q1.y * dx + q2.x * dy) + q2.y * dz) - lo;
                const double hc = ((q3.x * dx + q3.y * dy) + q4.x * dz) - lo;
                const double dn = (q4.y * dx + q5.x * dy) + q5.y * dz;
                const double dbl = q6.x, thr = q6.y;
                double top = ha > hb ? ha : hb;
                top = top > hc ? top : hc;
                const bool on_bed = top <= bed_tol;
                const bool over = !on_bed && dn < thr;                 // (a non-finite triangle: dn and thr are NaN)
                const bool contact = on_bed && dn < 0.0;
                s0 = s0 + (over ? dbl : 0.0);
                s1 = s1 + (over ? (-dn) * ((ha + hb) + hc) : 0.0);
                s2 = s2 + (contact ? dbl : 0.0);
                n_over += over ? 1u : 0u;
                n_contact += contact ? 1u : 0u;
            }
        }
    }
    if (active) {
        double *p = partials + (k * n_chunks + chunk) * OVERHANG_SUMS;
        p[0] = s0; p[1] = s1; p[2] = s2;
        packed[k * n_chunks + chunk] = n_over | (n_contact << 16);
    }
}

// grid: directions x groups of 256 partials (the group varies fastest); in[direction][n][SUMS] -> out[direction][n_groups][SUMS]
// (SUMS: the 3 totals of the rating, the 5 columns of the support rays below).
// packed != NULL (the first level): the chunks' packed counts of the group are added to counts[direction][2]
template <int SUMS>
__global__ __launch_bounds__(256) void k_overhang_partials(const double *__restrict__ in, long long n, unsigned n_groups, double *__restrict__ out,
                                                           const unsigned *__restrict__ packed, unsigned long long *__restrict__ counts) {
    __shared__ double tile[128 * SUMS];
    __shared__ unsigned wave_cnt[2][4];
    const int tid = (int)threadIdx.x;
    const long long dir = (long long)(blockIdx.x / n_groups), g = (long long)(blockIdx.x % n_groups);
    const long long i = g * 256 + tid;
    double acc[SUMS];
#pragma unroll
    for (int c = 0; c < SUMS; c++) acc[c] = i < n ? in[(dir * n + i) * SUMS + c] : 0.0;
    // (tree256 of sdf_block.h, spelt out: through the helper the kernel differs from its parent by one scalar instruction, and the
    // kernel is held to its parent's form, see below)
    for (int h = 128; h >= 64; h >>= 1) {                              // x[:h] + x[h:]: through LDS across the waves
        if (tid >= h && tid < 2 * h) {
#pragma unroll
            for (int c = 0; c < SUMS; c++) tile[c * 128 + (tid - h)] = acc[c];
        }
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int c = 0; c < SUMS; c++) acc[c] = acc[c] + tile[c * 128 + tid];
        }
        __syncthreads();
    }
    if (tid < 64) {                                                    // (wave 0, whole)
        for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
            for (int c = 0; c < SUMS; c++) acc[c] = acc[c] + __shfl_down(acc[c], h);
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < SUMS; c++) out[(dir * n_groups + g) * SUMS + c] = acc[c];
    }
    if (packed) {                                                      // (uniform; a group's counts stay below 2^18)
        const unsigned w = i < n ? packed[dir * n + i] : 0u;
        // (not block_add: with it a figure of the rating and one of the support rays lay above the parent's three runs)
        unsigned a = w & 0xffffu, b = w >> 16;
        for (int h = 32; h >= 1; h >>= 1) { a += __shfl_down(a, h); b += __shfl_down(b, h); }
        if ((tid & 63) == 0) { wave_cnt[0][tid >> 6] = a; wave_cnt[1][tid >> 6] = b; }
        __syncthreads();
        if (tid < 2) {
            const unsigned long long total = (unsigned long long)wave_cnt[tid][0] + wave_cnt[tid][1] + wave_cnt[tid][2] + wave_cnt[tid][3];
            if (total) atomicAdd(counts + 2 * dir + tid, total);
        }
    }
}

// one direction, one triangle per lane: 0 neither, 1 overhang, 2 bed contact, 3 non-finite
__global__ __launch_bounds__(256) void k_overhang_classes(const double *__restrict__ soup, long long n_tris, const double *__restrict__ dirs,
                                                          const unsigned long long *__restrict__ ext, double sin_limit, double bed_tol,
                                                          unsigned char *__restrict__ classes) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tris) return;
    const double dx = dirs[0], dy = dirs[1], dz = dirs[2], lo = box_value(ext[0]);
    double v[9], n[3], dbl;
#pragma unroll
    for (int c = 0; c < 9; c++) v[c] = soup[9 * t + c];
    const bool ok = triangle_parts(v, n, &dbl);
    const double ha = ((v[0] * dx + v[1] * dy) + v[2] * dz) - lo;
    const double hb = ((v[3] * dx + v[4] * dy) + v[5] * dz) - lo;
    const double hc = ((v[6] * dx + v[7] * dy) + v[8] * dz) - lo;
    const double dn = (n[0] * dx + n[1] * dy) + n[2] * dz;
    double top = ha > hb ? ha : hb;
    top = top > hc ? top : hc;
    const bool on_bed = top <= bed_tol;
    const bool over = !on_bed && dn < -(sin_limit * dbl), contact = on_bed && dn < 0.0;
    classes[t] = !ok ? 3 : over ? 1 : contact ? 2 : 0;
}

static unsigned extent_blocks(long long n_tris) {
    const long long n_tiles = (n_tris + OVERHANG_TILE - 1) / OVERHANG_TILE;
    return (unsigned)(n_tiles < EXTENT_MAX_BLOCKS ? n_tiles : EXTENT_MAX_BLOCKS);
}

int overhang_rate(hipStream_t st, const double *d_soup, long long n_tris, const double *h_dirs, long long n_dirs, double sin_limit,
                  double bed_tol, size_t max_scratch_bytes, double *h_values, int64_t *h_counts, long long *n_slabs, double *kernel_ms) {
    static const char who[] = "sdf_mesh_overhangs: ";
    if (n_tris < 1 || n_tris >= (1ll << 31)) return fail(std::string(who) + "the triangle count is out of range");
    if (n_dirs < 1 || n_dirs > OVERHANG_MAX_DIRS) return fail(std::string(who) + "the direction count is out of range");
    const long long n_chunks = (n_tris + OVERHANG_CHUNK - 1) / OVERHANG_CHUNK;      // (< 2^21)
    const long long n_second = (n_chunks + 255) / 256;
    // the slab: as many directions as keep the partials (two levels of sums, the packed counts) under the cap -- whole groups of 256
    // (or waves of 64) where that many fit, never fewer than one, and no more than a grid of workgroups can number
    const size_t per_dir = (size_t)n_chunks * (OVERHANG_SUMS * 8 + 4) + (size_t)n_second * OVERHANG_SUMS * 8;
    const size_t cap = max_scratch_bytes ? max_scratch_bytes : OVERHANG_SCRATCH_CAP;
    long long slab = (long long)(cap / per_dir);
    if (slab >= 256) slab &= ~255ll;
    else if (slab >= 64) slab &= ~63ll;
    if (slab < 1) slab = 1;
    const long long max_groups = ((1ll << 31) - 1) / n_chunks;         // (>= 1023)
    if (slab > max_groups * OVERHANG_TILE) slab = max_groups * OVERHANG_TILE;
    if (slab > n_dirs) slab = n_dirs;
    const size_t ns = (size_t)slab;
    std::vector<unsigned long long> h_ext(2 * (size_t)n_dirs), h_cnt(2 * (size_t)n_dirs);
    std::vector<double> h_sums(OVERHANG_SUMS * (size_t)n_dirs);
    std::deque<EventTimer> timers;
    double *d_dirs, *part_a, *part_b;
    unsigned long long *d_ext, *d_cnt;
    unsigned *d_packed;
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    scratch.part(&d_dirs, 3 * ns);
    scratch.part(&d_ext, 2 * ns);
    scratch.part(&d_cnt, 2 * ns);
    scratch.part(&part_a, ns * (size_t)n_chunks * OVERHANG_SUMS);
    scratch.part(&part_b, ns * (size_t)n_second * OVERHANG_SUMS);
    scratch.part(&d_packed, ns * (size_t)n_chunks);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    long long slabs = 0;
    for (long long k0 = 0; k0 < n_dirs; k0 += slab, slabs++) {
        const long long nk = n_dirs - k0 < slab ? n_dirs - k0 : slab;
        const unsigned n_dgroups = (unsigned)((nk + OVERHANG_TILE - 1) / OVERHANG_TILE);
        HIPCHK_MSG(who, hipMemcpyAsync(d_dirs, h_dirs + 3 * k0, (size_t)nk * 24, hipMemcpyHostToDevice, st));
        timers.emplace_back();
        EventTimer &timer = timers.back();
        HIPCHK_MSG(who, timer.start(st));
        HIPCHK_MSG(who, launch_rows(k_overhang_init, nk, st, nk, d_ext, d_cnt));
        HIPCHK_MSG(who, launch_grid(k_overhang_extents, extent_blocks(n_tris) * n_dgroups, st, d_soup, n_tris, d_dirs, nk, n_dgroups, d_ext));
        HIPCHK_MSG(who, launch_grid(k_overhang_terms, (unsigned)(n_chunks * n_dgroups), st, d_soup, n_tris, d_dirs, nk, n_dgroups, n_chunks, d_ext,
                                    sin_limit, bed_tol, part_a, d_packed));
        double *src = part_a, *dst = part_b;
        bool first = true;
        for (long long n = n_chunks; first || n > 1; n = (n + 255) / 256, first = false) {             // 256 partials to one, until one is left
            const unsigned n_groups = (unsigned)((n + 255) / 256);
            HIPCHK_MSG(who, launch_grid(k_overhang_partials<OVERHANG_SUMS>, (unsigned)(nk * n_groups), st, src, n, n_groups, dst, first ? d_packed : nullptr, d_cnt));
            double *t = src; src = dst; dst = t;
        }
        HIPCHK_MSG(who, timer.stop(st));
        HIPCHK_MSG(who, hipMemcpyAsync(h_sums.data() + OVERHANG_SUMS * k0, src, (size_t)nk * OVERHANG_SUMS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK_MSG(who, hipMemcpyAsync(h_ext.data() + 2 * k0, d_ext, (size_t)nk * 16, hipMemcpyDeviceToHost, st));
        HIPCHK_MSG(who, hipMemcpyAsync(h_cnt.data() + 2 * k0, d_cnt, (size_t)nk * 16, hipMemcpyDeviceToHost, st));
    }
    HIPCHK_MSG(who, stream_wait(st));
    double total_ms = 0.0;
    for (EventTimer &t : timers) {
        double ms = 0.0;
        HIPCHK_MSG(who, t.ms(&ms));
        total_ms += ms;
    }
    *kernel_ms = total_ms;
    *n_slabs = slabs;
    for (long long k = 0; k < n_dirs; k++) {
        h_values[5 * k] = box_value(h_ext[2 * k]);
        h_values[5 * k + 1] = box_value(h_ext[2 * k + 1]);
        for (int c = 0; c < OVERHANG_SUMS; c++) h_values[5 * k + 2 + c] = h_sums[OVERHANG_SUMS * k + c];
        h_counts[2 * k] = (int64_t)h_cnt[2 * k];
        h_counts[2 * k + 1] = (int64_t)h_cnt[2 * k + 1];
    }
    return 0;
}

int overhang_classes(hipStream_t st, const double *d_soup, long long n_tris, const double *h_dir3, double sin_limit, double bed_tol,
                     uint8_t *h_classes, double *kernel_ms) {
    static const char who[] = "sdf_mesh_overhang_classes: ";
    if (n_tris < 1 || n_tris >= (1ll << 31)) return fail(std::string(who) + "the triangle count is out of range");
    double *d_dirs;
    unsigned long long *d_ext, *d_cnt;
    unsigned char *d_classes;
    Scratch scratch(st);
    scratch.part(&d_dirs, 3);
    scratch.part(&d_ext, 2);
    scratch.part(&d_cnt, 2);
    scratch.part(&d_classes, (size_t)n_tris);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    HIPCHK_MSG(who, hipMemcpyAsync(d_dirs, h_dir3, 24, hipMemcpyHostToDevice, st));
    EventTimer timer;
    HIPCHK_MSG(who, timer.start(st));
    HIPCHK_MSG(who, launch_rows(k_overhang_init, 1, st, 1, d_ext, d_cnt));
    HIPCHK_MSG(who, launch_grid(k_overhang_extents, extent_blocks(n_tris), st, d_soup, n_tris, d_dirs, 1, 1, d_ext));
    HIPCHK_MSG(who, launch_rows(k_overhang_classes, n_tris, st, d_soup, n_tris, d_dirs, d_ext, sin_limit, bed_tol, d_classes));
    HIPCHK_MSG(who, timer.stop(st));
    HIPCHK_MSG(who, hipMemcpyAsync(h_classes, d_classes, (size_t)n_tris, hipMemcpyDeviceToHost, st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, timer.ms(kernel_ms));
    return 0;
}

// ---- support rays: everything of a call but the rays themselves, which are a tape interpreter and live in
// sdf_supports.hip.  The faces are the class-1 triangles of k_overhang_classes above, numbered in triangle order by the scan of
// sdf_prims.hip; the sums run over the RAYS in that order through the same tree as the rating's. ----

// one triangle per lane: the flag the scan numbers
__global__ __launch_bounds__(256) void k_support_flags(const unsigned char *__restrict__ classes, long long n_tris, int *__restrict__ flags) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n_tris) flags[t] = classes[t] == 1 ? 1 : 0;
}

// one triangle per lane: an overhanging one writes its index at its number
__global__ __launch_bounds__(256) void k_support_number(const int *__restrict__ flags, const int *__restrict__ pos, long long n_tris, long long m,
                                                        int32_t *__restrict__ triangle) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tris || !flags[t]) return;
    const long long r = pos[t];
    if (r >= 0 && r < m) triangle[r] = (int32_t)t;
}

// one lane per (chunk of 1024 rays, column): ONE accumulator walks its run of the column in index order from +0.0 -- eight loads in
// flight, then their terms IN ORDER (k_contour_area's pattern).  terms: column c at terms + c * m; partials[chunk][SUPPORT_SUMS]
__global__ __launch_bounds__(256) void k_support_chunks(const double *__restrict__ terms, long long m, long long n_chunks, double *__restrict__ partials) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_chunks * SUPPORT_SUMS) return;
    const long long chunk = g / SUPPORT_SUMS, col = g - chunk * SUPPORT_SUMS;
    const double *p = terms + col * m;
    const long long i0 = chunk * OVERHANG_CHUNK, i1 = i0 + OVERHANG_CHUNK < m ? i0 + OVERHANG_CHUNK : m;
    double acc = 0.0;
    long long i = i0;
    for (; i + 8 <= i1; i += 8) {
        double q[8];
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = p[i + k];
#pragma unroll
        for (int k = 0; k < 8; k++) acc = acc + q[k];
    }
    for (; i < i1; i++) acc = acc + p[i];
    partials[g] = acc;
}

// one ray per lane: the rays of each status, one integer atomic per workgroup and counter
__global__ __launch_bounds__(256) void k_support_counts(const unsigned char *__restrict__ status, long long m, unsigned long long *__restrict__ counts) {
    // (not block_count: with it a figure of the support rays lay above the parent's three runs)
    __shared__ unsigned wave_cnt[SUPPORT_STATUSES][4];
    const int tid = (int)threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const int s = i < m ? (int)status[i] : -1;
#pragma unroll
    for (int c = 0; c < SUPPORT_STATUSES; c++) {
        const unsigned n = (unsigned)__popcll(__ballot(s == c));
        if ((tid & 63) == 0) wave_cnt[c][tid >> 6] = n;
    }
    __syncthreads();
    if (tid < SUPPORT_STATUSES) {
        const unsigned long long total = (unsigned long long)wave_cnt[tid][0] + wave_cnt[tid][1] + wave_cnt[tid][2] + wave_cnt[tid][3];
        if (total) atomicAdd(counts + tid, total);
    }
}

int support_rays_run(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *d_soup, long long n_tris,
                     const double *h_dirs, long long n_dirs, const SupportParams &p, std::vector<SupportRaysDir> *out, double *h_values,
                     int64_t *h_counts, double *parts_ms4) {
    static const char who[] = "sdf_mesh_support_rays: ";
    if (n_tris < 1 || n_tris >= (1ll << 31)) return fail(std::string(who) + "the triangle count is out of range");
    if (n_dirs < 1 || n_dirs > SUPPORT_MAX_DIRS) return fail(std::string(who) + "the direction count is out of range");
    const size_t nt = (size_t)n_tris;
    const long long max_chunks = (n_tris + OVERHANG_CHUNK - 1) / OVERHANG_CHUNK, max_second = (max_chunks + 255) / 256;
    size_t tmp_bytes = 0;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n_tris, &tmp_bytes));
    std::vector<unsigned long long> h_ext(2 * (size_t)n_dirs), h_cnt(SUPPORT_STATUSES * (size_t)n_dirs, 0ull);
    std::vector<double> h_sums(SUPPORT_SUMS * (size_t)n_dirs, 0.0);
    std::deque<EventTimer> timers;
    double *d_dir, *terms, *part_a, *part_b;
    unsigned long long *d_ext, *d_cnt2, *d_counts;
    unsigned char *d_classes, *tmp;
    int *flags, *pos;
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    scratch.part(&d_dir, 3);
    scratch.part(&d_ext, 2);
    scratch.part(&d_cnt2, 2);
    scratch.part(&d_counts, SUPPORT_STATUSES);
    scratch.part(&d_classes, nt);
    scratch.part(&flags, nt);
    scratch.part(&pos, nt);
    scratch.part(&tmp, tmp_bytes);
    scratch.part(&terms, nt * SUPPORT_SUMS);
    scratch.part(&part_a, (size_t)max_chunks * SUPPORT_SUMS);
    scratch.part(&part_b, (size_t)max_second * SUPPORT_SUMS);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    out->clear();
    out->resize((size_t)n_dirs);
    for (long long k = 0; k < n_dirs; k++) {
        SupportRaysDir &res = (*out)[(size_t)k];
        timers.emplace_back(); EventTimer &t_classes = timers.back();
        timers.emplace_back(); EventTimer &t_number = timers.back();
        HIPCHK_MSG(who, hipMemcpyAsync(d_dir, h_dirs + 3 * k, 24, hipMemcpyHostToDevice, st));
        HIPCHK_MSG(who, t_classes.start(st));
        HIPCHK_MSG(who, launch_rows(k_overhang_init, 1, st, 1, d_ext, d_cnt2));
        HIPCHK_MSG(who, launch_grid(k_overhang_extents, extent_blocks(n_tris), st, d_soup, n_tris, d_dir, 1, 1, d_ext));
        HIPCHK_MSG(who, launch_rows(k_overhang_classes, n_tris, st, d_soup, n_tris, d_dir, d_ext, p.sin_limit, p.bed_tol, d_classes));
        HIPCHK_MSG(who, t_classes.stop(st));
        HIPCHK_MSG(who, hipMemcpyAsync(h_ext.data() + 2 * k, d_ext, 16, hipMemcpyDeviceToHost, st));      // (lands behind the scan's wait)
        HIPCHK_MSG(who, t_number.start(st));
        HIPCHK_MSG(who, launch_rows(k_support_flags, n_tris, st, d_classes, n_tris, flags));
        long long m = 0;
        if (number_flags(who, "overhang flags", st, flags, pos, n_tris, tmp, tmp_bytes, &m)) return 1;
        res.m = m;
        if (m < 1) {
            HIPCHK_MSG(who, t_number.stop(st));
            continue;
        }
        // the direction's block: origin, height, triangle, steps, status
        const size_t nm = (size_t)m;
        res.o_height = align256(nm * 24);
        res.o_triangle = res.o_height + align256(nm * 8);
        res.o_steps = res.o_triangle + align256(nm * 4);
        res.o_status = res.o_steps + align256(nm * 4);
        const size_t bytes = res.o_status + align256(nm);
        HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(bytes) + "): ", res.block.alloc(bytes, st));
        char *base = res.block.as<char>();
        double *origin = (double *)base, *height = (double *)(base + res.o_height);
        int32_t *triangle = (int32_t *)(base + res.o_triangle), *steps = (int32_t *)(base + res.o_steps);
        uint8_t *status = (uint8_t *)(base + res.o_status);
        HIPCHK_MSG(who, launch_rows(k_support_number, n_tris, st, flags, pos, n_tris, m, triangle));
        HIPCHK_MSG(who, t_number.stop(st));
        timers.emplace_back(); EventTimer &t_rays = timers.back();
        timers.emplace_back(); EventTimer &t_sums = timers.back();
        SupportArgs a;
        a.dx = h_dirs[3 * k]; a.dy = h_dirs[3 * k + 1]; a.dz = h_dirs[3 * k + 2];
        a.lo = box_value(h_ext[2 * (size_t)k]);
        a.start = p.start; a.min_step = p.min_step; a.step_scale = p.step_scale; a.max_steps = p.max_steps; a.refine = p.refine;
        HIPCHK_MSG(who, t_rays.start(st));
        HIPCHK_MSG(who, (hipError_t)launch_support_rays(st, d_code, d_consts, full, d_soup, triangle, m, a, height, status, steps, origin, terms));
        HIPCHK_MSG(who, t_rays.stop(st));
        HIPCHK_MSG(who, t_sums.start(st));
        const long long n_chunks = (m + OVERHANG_CHUNK - 1) / OVERHANG_CHUNK;
        HIPCHK_MSG(who, launch_rows(k_support_chunks, n_chunks * SUPPORT_SUMS, st, terms, m, n_chunks, part_a));
        double *src = part_a, *dst = part_b;
        bool first = true;
        for (long long n = n_chunks; first || n > 1; n = (n + 255) / 256, first = false) {             // 256 partials to one, until one is left
            const unsigned n_groups = (unsigned)((n + 255) / 256);
            HIPCHK_MSG(who, launch_grid(k_overhang_partials<SUPPORT_SUMS>, n_groups, st, src, n, n_groups, dst, nullptr, nullptr));
            double *t = src; src = dst; dst = t;
        }
        HIPCHK_MSG(who, hipMemsetAsync(d_counts, 0, SUPPORT_STATUSES * 8, st));
        HIPCHK_MSG(who, launch_rows(k_support_counts, m, st, status, m, d_counts));
        HIPCHK_MSG(who, t_sums.stop(st));
        HIPCHK_MSG(who, hipMemcpyAsync(h_sums.data() + SUPPORT_SUMS * k, src, SUPPORT_SUMS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK_MSG(who, hipMemcpyAsync(h_cnt.data() + SUPPORT_STATUSES * k, d_counts, SUPPORT_STATUSES * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK_MSG(who, stream_wait(st));
    for (int c = 0; c < 4; c++) parts_ms4[c] = 0.0;
    {
        size_t ti = 0;
        for (long long k = 0; k < n_dirs; k++) {
            const int n = (*out)[(size_t)k].m > 0 ? 4 : 2;
            for (int c = 0; c < n; c++, ti++) {
                double ms = 0.0;
                HIPCHK_MSG(who, timers[ti].ms(&ms));
                parts_ms4[c] += ms;
            }
        }
    }
    for (long long k = 0; k < n_dirs; k++) {
        h_values[7 * k] = box_value(h_ext[2 * k]);
        h_values[7 * k + 1] = box_value(h_ext[2 * k + 1]);
        for (int c = 0; c < SUPPORT_SUMS; c++) h_values[7 * k + 2 + c] = h_sums[SUPPORT_SUMS * k + c];
        for (int c = 0; c < SUPPORT_STATUSES; c++) h_counts[6 * k + c] = (int64_t)h_cnt[SUPPORT_STATUSES * k + c];
        h_counts[6 * k + 5] = (int64_t)(*out)[(size_t)k].m;
    }
    return 0;
}

}  // namespace sdfk
