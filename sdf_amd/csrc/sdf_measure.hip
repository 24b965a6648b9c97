// sdf_measure.hip -- a mesh measured where it lies (sdf_mesh_moments, sdf_mesh_edge_census, ABI 15).
// tests/measure_ref.py is the definition; these kernels reproduce it bit for bit: float64, one rounding per written operation
// (-ffp-contract=off), and a summation TREE that depends on the order of the triangles and on nothing else.
//
// Moments.  The soup is cut into chunks of MOMENT_CHUNK = 1024 consecutive triangles, one workgroup of 256 lanes each.  A chunk is
// read as four tiles of 256 triangles: the tile's 18432 contiguous bytes go into LDS by 16-byte loads (a lane's own 72-byte record
// is not a coalesced access), lane l takes triangle l of the tile from there and adds its 11 terms to accumulators that start at
// +0.0 -- so lane l adds triangles l, l + 256, l + 512, l + 768 of the chunk in index order.  Then the halving tree x[:h] + x[h:],
// h = 128 ... 1: through LDS across the waves (h = 128, 64), by cross-lane moves inside wave 0 (h = 32 ... 1).  The chunk partials
// go through k_moment_partials -- one partial per lane, the same tree -- 256 to one per launch until one is left.  A missing
// triangle or partial is +0.0; an accumulator never holds -0.0 (it starts at +0.0 and x + y is -0.0 only for two -0.0), so skipping
// the padding adds nothing.  No floating-point atomics: the two counters and the bounding box (on keys whose unsigned order is the
// float order) use integer ones.
//
// Census.  k_edge_keys writes three u64 keys per cell, min * 2^32 + max * 2 + dir, all ones for a collapsed cell; a library radix
// sort (hipCUB, like the weld's); k_edge_classes gives every sorted key a lane: the key that starts a run of one undirected edge
// looks two keys ahead -- run length 1, 2, "3 or more" and two direction bits decide the class -- so no lane walks a long run.
// The counters are integer atomics, one per workgroup and class.
//
// The tree, the box reduced across a workgroup, its keys and the counters' sums are sdf_block.h's.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <string>

#include "sdf_block.h"
#include "sdf_measure.h"
#include "sdf_runtime.h"

namespace sdfk {

constexpr int MOMENT_SUMS = 11;
constexpr int MOMENT_TILE = 256;                   // triangles per tile = lanes per workgroup
constexpr int MOMENT_CHUNK = 1024;                 // triangles per chunk (tests/measure_ref.py: C)
constexpr int BOX_MAX_BLOCKS = 1024;                 // workgroups that stride over the soup (k_soup_box) or the keys (k_edge_classes)
constexpr unsigned long long EDGE_COLLAPSED = ~0ull;

// triangles [t0, t0 + cnt) of the soup into LDS, contiguous: 16-byte loads where the soup's base allows them
template <bool WIDE>
__device__ __forceinline__ void stage_tile(const double *__restrict__ soup, long long t0, int cnt, double *tile) {
    const double *src = soup + 9 * t0;
    const int nd = 9 * cnt, tid = (int)threadIdx.x;
    if (WIDE) {                                                        // (9 * 256 * 8 bytes per tile: every tile starts 16-byte aligned)
        const double2 *s2 = reinterpret_cast<const double2 *>(src);
        double2 *l2 = reinterpret_cast<double2 *>(tile);
#pragma unroll 5
        for (int j = tid; j < nd / 2; j += MOMENT_TILE) l2[j] = s2[j];
        if ((nd & 1) && tid == 0) tile[nd - 1] = src[nd - 1];          // (an odd count: the last double alone, nothing is read past the soup)
    } else {
        for (int j = tid; j < nd; j += MOMENT_TILE) tile[j] = src[j];
    }
}

// the bounding box of the triangles whose vertices are all finite, on box_key's keys: box[0..2] min, box[3..5] max
template <bool WIDE>
__global__ __launch_bounds__(256) void k_soup_box(const double *__restrict__ soup, long long n_tris, unsigned long long *__restrict__ box) {
    __shared__ __attribute__((aligned(16))) double tile[9 * MOMENT_TILE];
    const int tid = (int)threadIdx.x;
    const long long n_tiles = (n_tris + MOMENT_TILE - 1) / MOMENT_TILE;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    for (long long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const long long t0 = tl * MOMENT_TILE;
        const int cnt = (int)(n_tris - t0 < MOMENT_TILE ? n_tris - t0 : MOMENT_TILE);
        __syncthreads();
        stage_tile<WIDE>(soup, t0, cnt, tile);
        __syncthreads();
        if (tid < cnt) {
            double v[9];
#pragma unroll
            for (int k = 0; k < 9; k++) v[k] = tile[9 * tid + k];
            if (finite9(v)) {
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const unsigned long long key = box_key(v[k]);
                    lo[k % 3] = key < lo[k % 3] ? key : lo[k % 3];
                    hi[k % 3] = key > hi[k % 3] ? key : hi[k % 3];
                }
            }
        }
    }
    wave_box_min_max(lo, hi);
    block_box_merge(lo, hi, box);
}

// one chunk of MOMENT_CHUNK triangles per workgroup: partials[chunk][11]; counts[0] += zero-area, counts[1] += non-finite triangles
template <bool WIDE>
__global__ __launch_bounds__(256) void k_soup_moments(const double *__restrict__ soup, long long n_tris, const unsigned long long *__restrict__ box,
                                                      double o0, double o1, double o2, int origin_from_box, double *__restrict__ partials,
                                                      unsigned long long *__restrict__ counts, double *__restrict__ origin_out) {
    __shared__ __attribute__((aligned(16))) double tile[9 * MOMENT_TILE];
    const int tid = (int)threadIdx.x;
    if (origin_from_box) {                                             // lo + (hi - lo) / 2; an empty box: (0, 0, 0)
        double o[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned long long kl = box[k], kh = box[3 + k];
            const double lo = box_value(kl), hi = box_value(kh);
            o[k] = kl > kh ? 0.0 : lo + (hi - lo) / 2.0;
        }
        o0 = o[0]; o1 = o[1]; o2 = o[2];
    }
    if (blockIdx.x == 0 && tid == 0) { origin_out[0] = o0; origin_out[1] = o1; origin_out[2] = o2; }
    double acc[MOMENT_SUMS];
#pragma unroll
    for (int k = 0; k < MOMENT_SUMS; k++) acc[k] = 0.0;
    unsigned n_zero = 0, n_bad = 0;                                    // (per wave: lane 0 of each wave keeps them)
    const long long c0 = (long long)blockIdx.x * MOMENT_CHUNK;
#pragma unroll 1
    for (int s = 0; s < MOMENT_CHUNK / MOMENT_TILE; s++) {
        const long long t0 = c0 + (long long)s * MOMENT_TILE;
        if (t0 >= n_tris) break;                                       // (uniform)
        const int cnt = (int)(n_tris - t0 < MOMENT_TILE ? n_tris - t0 : MOMENT_TILE);
        __syncthreads();
        stage_tile<WIDE>(soup, t0, cnt, tile);
        __syncthreads();
        bool zero = false, bad = false;
        if (tid < cnt) {
            double v[9];
#pragma unroll
            for (int k = 0; k < 9; k++) v[k] = tile[9 * tid + k];
            bad = !finite9(v);
            if (!bad) {
                const double ax = v[0] - o0, ay = v[1] - o1, az = v[2] - o2;
                const double bx = v[3] - o0, by = v[4] - o1, bz = v[5] - o2;
                const double cx = v[6] - o0, cy = v[7] - o1, cz = v[8] - o2;
                const double ux = bx - ax, uy = by - ay, uz = bz - az;
                const double wx = cx - ax, wy = cy - ay, wz = cz - az;
                const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                const double dbl = sqrt((nx * nx + ny * ny) + nz * nz);
                zero = dbl == 0.0;
                const double mx = by * cz - bz * cy, my = bz * cx - bx * cz, mz = bx * cy - by * cx;
                const double det = (ax * mx + ay * my) + az * mz;
                const double sx = (ax + bx) + cx, sy = (ay + by) + cy, sz = (az + bz) + cz;
                acc[0] = acc[0] + dbl;
                acc[1] = acc[1] + det;
                acc[2] = acc[2] + det * sx;
                acc[3] = acc[3] + det * sy;
                acc[4] = acc[4] + det * sz;
                acc[5] = acc[5] + det * (((ax * ax + bx * bx) + cx * cx) + sx * sx);
                acc[6] = acc[6] + det * (((ay * ay + by * by) + cy * cy) + sy * sy);
                acc[7] = acc[7] + det * (((az * az + bz * bz) + cz * cz) + sz * sz);
                acc[8] = acc[8] + det * (((ax * ay + bx * by) + cx * cy) + sx * sy);
                acc[9] = acc[9] + det * (((ax * az + bx * bz) + cx * cz) + sx * sz);
                acc[10] = acc[10] + det * (((ay * az + by * bz) + cy * cz) + sy * sz);
            }
        }
        n_zero += (unsigned)__popcll(__ballot(zero));
        n_bad += (unsigned)__popcll(__ballot(bad));
    }
    __syncthreads();                                                   // (the last tile has been read: the tree takes the LDS over)
    tree256<MOMENT_SUMS>(acc, tile);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < MOMENT_SUMS; k++) partials[(long long)blockIdx.x * MOMENT_SUMS + k] = acc[k];
    }
    if ((tid & 63) == 0) {                                             // one integer atomic per wave that has any
        if (n_zero) atomicAdd(counts, (unsigned long long)n_zero);
        if (n_bad) atomicAdd(counts + 1, (unsigned long long)n_bad);
    }
}

// 256 partials to one per workgroup, one partial per lane, the same tree
__global__ __launch_bounds__(256) void k_moment_partials(const double *__restrict__ in, long long n, double *__restrict__ out) {
    __shared__ double tile[128 * MOMENT_SUMS];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    double acc[MOMENT_SUMS];
#pragma unroll
    for (int k = 0; k < MOMENT_SUMS; k++) acc[k] = i < n ? in[i * MOMENT_SUMS + k] : 0.0;
    tree256<MOMENT_SUMS>(acc, tile);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MOMENT_SUMS; k++) out[(long long)blockIdx.x * MOMENT_SUMS + k] = acc[k];
    }
}

// one lane per cell: three half-edge keys, min * 2^32 + max * 2 + (1 when the half-edge runs from max to min); a cell with two
// equal indices is collapsed: three sentinels, and it is counted
__global__ __launch_bounds__(256) void k_edge_keys(const long long *__restrict__ cells, long long n_tris, unsigned long long *__restrict__ keys,
                                                   unsigned long long *__restrict__ n_collapsed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_tris;
    bool collapsed = false;
    if (live) {
        const unsigned long long c[3] = {(unsigned long long)cells[3 * i], (unsigned long long)cells[3 * i + 1], (unsigned long long)cells[3 * i + 2]};
        collapsed = c[0] == c[1] || c[1] == c[2] || c[2] == c[0];
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const unsigned long long u = c[e], v = c[(e + 1) % 3];
            const unsigned long long lo = u < v ? u : v, hi = u < v ? v : u;
            keys[3 * i + e] = collapsed ? EDGE_COLLAPSED : (lo << 32) + hi * 2ull + (u > v ? 1ull : 0ull);
        }
    }
    wave_add(wave_count(collapsed), n_collapsed);
}

// one lane per sorted key, a workgroup strides over the keys; classes[0..3] += paired, boundary, misoriented, non-manifold edges.
// Every lane counts in registers; block_add (sdf_block.h) sends one integer atomic per workgroup and class that has any.
__global__ __launch_bounds__(256) void k_edge_classes(const unsigned long long *__restrict__ keys, long long n, unsigned long long *__restrict__ classes) {
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned long long k = keys[i];
        const unsigned long long e = k >> 1;
        if (k != EDGE_COLLAPSED && (i == 0 || (keys[i - 1] >> 1) != e)) {               // the first use of an undirected edge
            const bool two = i + 1 < n && (keys[i + 1] >> 1) == e;
            const bool three = two && i + 2 < n && (keys[i + 2] >> 1) == e;
            const int cls = three ? 3 : !two ? 1 : ((k ^ keys[i + 1]) & 1ull) ? 0 : 2;
#pragma unroll
            for (int c = 0; c < 4; c++) cnt[c] += cls == c ? 1u : 0u;
        }
    }
    block_add(cnt, classes);
}

int measure_moments(hipStream_t st, const double *d_soup, long long n_tris, const double *origin, sdf_moments *out, double *kernel_ms) {
    static const char who[] = "sdf_mesh_moments: ";
    const long long n_chunks = (n_tris + MOMENT_CHUNK - 1) / MOMENT_CHUNK;
    if (n_tris < 1 || n_chunks >= (1ll << 31)) return fail(std::string(who) + "the triangle count is out of range");
    const long long n_second = (n_chunks + 255) / 256;
    // what comes back: [11 sums | origin 3] as doubles, [box 6 | counts 2] as u64 -- `head` is both the device block and its copy here
    struct Head { double origin[3]; unsigned long long box[6]; unsigned long long counts[2]; } h_head;
    double h_sums[MOMENT_SUMS];
    Head *d_head;
    double *part_a, *part_b;
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    scratch.part(&d_head, 1);
    scratch.part(&part_a, (size_t)n_chunks * MOMENT_SUMS);
    scratch.part(&part_b, (size_t)n_second * MOMENT_SUMS);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    for (int k = 0; k < 3; k++) { h_head.origin[k] = 0.0; h_head.box[k] = BOX_EMPTY_LO; h_head.box[3 + k] = BOX_EMPTY_HI; }
    h_head.counts[0] = h_head.counts[1] = 0;
    HIPCHK_MSG(who, hipMemcpyAsync(d_head, &h_head, sizeof(Head), hipMemcpyHostToDevice, st));
    const bool wide = (reinterpret_cast<uintptr_t>(d_soup) & 15u) == 0;
    const long long n_tiles = (n_tris + MOMENT_TILE - 1) / MOMENT_TILE;
    const unsigned box_grid = (unsigned)(n_tiles < BOX_MAX_BLOCKS ? n_tiles : BOX_MAX_BLOCKS);
    const double o0 = origin ? origin[0] : 0.0, o1 = origin ? origin[1] : 0.0, o2 = origin ? origin[2] : 0.0;
    EventTimer timer;
    HIPCHK_MSG(who, timer.start(st));
    HIPCHK_MSG(who, launch_grid(wide ? k_soup_box<true> : k_soup_box<false>, box_grid, st, d_soup, n_tris, d_head->box));
    HIPCHK_MSG(who, launch_grid(wide ? k_soup_moments<true> : k_soup_moments<false>, (unsigned)n_chunks, st, d_soup, n_tris, d_head->box, o0, o1, o2,
                                origin ? 0 : 1, part_a, d_head->counts, d_head->origin));
    double *src = part_a, *dst = part_b;
    for (long long n = n_chunks; n > 1; n = (n + 255) / 256) {         // 256 partials to one, until one is left
        HIPCHK_MSG(who, launch_rows(k_moment_partials, n, st, src, n, dst));
        double *t = src; src = dst; dst = t;
    }
    HIPCHK_MSG(who, timer.stop(st));
    HIPCHK_MSG(who, hipMemcpyAsync(h_sums, src, sizeof(h_sums), hipMemcpyDeviceToHost, st));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, d_head, sizeof(Head), hipMemcpyDeviceToHost, st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, timer.ms(kernel_ms));
    for (int k = 0; k < MOMENT_SUMS; k++) out->sums[k] = h_sums[k];
    for (int k = 0; k < 3; k++) {
        out->origin[k] = h_head.origin[k];
        out->box_lo[k] = box_value(h_head.box[k]);
        out->box_hi[k] = box_value(h_head.box[3 + k]);
    }
    out->n_triangles = (int64_t)n_tris;
    out->n_zero_area = (int64_t)h_head.counts[0];
    out->n_nonfinite = (int64_t)h_head.counts[1];
    return 0;
}

int measure_edge_census(hipStream_t st, const long long *d_cells, long long n_tris, long long n_vertices, sdf_edge_census *out,
                        double *kernel_ms) {
    static const char who[] = "sdf_mesh_edge_census: ";
    const long long n = 3 * n_tris;
    if (n_tris < 1 || n >= (1ll << 31) || n_vertices >= (1ll << 31)) return fail(std::string(who) + "2^31 or more half-edges or vertices");
    unsigned long long h_counts[5] = {0, 0, 0, 0, 0};                  // collapsed, then the four classes
    unsigned long long *k0, *k1, *d_counts;
    unsigned char *tmp;
    size_t tmp_bytes = 0;
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)n, 0, 64, st));
    Scratch scratch(st);
    scratch.part(&k0, (size_t)n);
    scratch.part(&k1, (size_t)n);
    scratch.part(&tmp, tmp_bytes ? tmp_bytes : 1);
    scratch.part(&d_counts, 5);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    HIPCHK_MSG(who, hipMemsetAsync(d_counts, 0, sizeof(h_counts), st));
    EventTimer timer;
    HIPCHK_MSG(who, timer.start(st));
    HIPCHK_MSG(who, launch_rows(k_edge_keys, n_tris, st, d_cells, n_tris, k0, d_counts));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, (const unsigned long long *)k0, k1, (int)n, 0, 64, st));
    HIPCHK_MSG(who, launch_grid(k_edge_classes, blocks_of(n) < BOX_MAX_BLOCKS ? blocks_of(n) : BOX_MAX_BLOCKS, st, k1, n, d_counts + 1));
    HIPCHK_MSG(who, timer.stop(st));
    HIPCHK_MSG(who, hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, timer.ms(kernel_ms));
    out->vertices = (int64_t)n_vertices;
    out->collapsed = (int64_t)h_counts[0];
    out->faces = (int64_t)n_tris - out->collapsed;
    out->paired = (int64_t)h_counts[1];
    out->boundary = (int64_t)h_counts[2];
    out->misoriented = (int64_t)h_counts[3];
    out->nonmanifold = (int64_t)h_counts[4];
    out->edges = out->paired + out->boundary + out->misoriented + out->nonmanifold;
    out->euler = out->vertices - out->edges + out->faces;
    out->closed = (out->boundary == 0 && out->nonmanifold == 0) ? 1 : 0;
    out->oriented = out->misoriented == 0 ? 1 : 0;
    return 0;
}

}  // namespace sdfk
