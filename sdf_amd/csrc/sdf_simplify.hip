// sdf_simplify.hip -- a welded mesh simplified on the device (sdf_mesh_simplify, ABI 17): Rossignac-Borrel
// vertex clustering on a uniform grid with one representative per cluster placed by a quadric error function (Lindstrom's
// out-of-core simplification).  tests/simplify_ref.py is the definition, and what is written here copies its float64 operations one
// by one, in its order: this unit is built with -ffp-contract=off, like sdf_measure.hip, and nothing below is fused.
//
// The passes.  k_cluster_box: one lane per welded vertex, the floor of its grid coordinates as ordered integer keys (box_key of
// sdf_measure.h), reduced across the workgroup, six integer atomics per workgroup; it also counts the vertices that are not finite.
// The host reads the box and refuses a mesh the keys cannot hold.  k_cluster_keys: one lane per vertex, the 63-bit key.  A stable
// library sort (hipCUB, like the weld's) of (key, welded index), adjacent-difference flags and a library exclusive scan number the
// clusters by ascending key: k_cluster_number writes the cluster of every vertex, the key of every cluster and where its run of the
// sorted vertices starts -- inside a run the welded indices ascend, because the sort is stable.  k_cluster_items: one lane per
// (triangle, corner) writes (cluster, item); a second stable library sort by cluster and k_item_starts give every cluster its run of
// items, in ascending item index.
//
// k_cluster_vertex: ONE LANE PER CLUSTER.  It walks its run of vertices for the mean and its run of items for the six + three sums
// of the quadric, gathering the three welded points of the item's triangle through the cells, solves the regularised 3 x 3 system
// by cofactors and applies the fallbacks.  Every float sum is sequential in the definition's order -- that is why a cluster is one
// lane and not a reduction tree: the result does not depend on the launch geometry, and no float atomic exists anywhere here.  The
// gathers are element-granular and rely on L2: welded order is lexicographic, so the points of one cell and of its neighbours lie in
// a few short runs of the array; the lanes of a wave are neighbouring clusters along z and share most of those lines.  A cluster
// whose runs are thousands of entries long is legal and slow for its lane only.  The two counters (flat, mean_fallback) are summed
// across the workgroup and added with one 64-bit integer atomic per workgroup.
//
// k_cluster_live flags the triangles whose three clusters differ, a library exclusive scan places them, and k_cluster_emit runs one
// lane per double of the output's source triangle, as k_select_copy does, so that the stores of a wave are contiguous.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>

#include "sdf_measure.h"
#include "sdf_prims.h"
#include "sdf_simplify.h"

namespace sdfk {

constexpr int KEY_BITS = 21;                         // bits of the key per axis: x << 42 | y << 21 | z
constexpr unsigned long long KEY_MASK = (1ull << KEY_BITS) - 1;

struct SimplifyGrid {
    double origin[3], cell[3], fqmin[3];             // fqmin: the per-axis minimum of floor((p - origin) / cell), known after the box pass
    long long qmin[3];
    double reg;
};

// what the box pass and the vertex pass leave for the host
struct SimplifyHead {
    unsigned long long box[6];                       // box_key of the floors: lo x, y, z, hi x, y, z
    unsigned long long counters;                     // flat << 32 | mean_fallback
    unsigned n_bad, pad;                             // vertices that are not finite
};

__global__ void k_cluster_head_init(SimplifyHead *head) {
    if (threadIdx.x < 3) { head->box[threadIdx.x] = ~0ull; head->box[3 + threadIdx.x] = 0ull; }
    if (threadIdx.x == 0) { head->counters = 0ull; head->n_bad = 0u; head->pad = 0u; }
}

__device__ __forceinline__ double grid_floor(double p, double origin, double cell) { return floor((p - origin) / cell); }

__global__ __launch_bounds__(256) void k_cluster_box(const double *__restrict__ pts, long long n, SimplifyGrid g, SimplifyHead *head) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    bool bad = false;
    if (v < n) {
        const double p[3] = {pts[3 * v], pts[3 * v + 1], pts[3 * v + 2]};
        bad = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
        if (!bad) {
#pragma unroll
            for (int c = 0; c < 3; c++) lo[c] = hi[c] = box_key(grid_floor(p[c], g.origin[c], g.cell[c]));
        }
    }
    for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const unsigned long long a = __shfl_down(lo[c], h), b = __shfl_down(hi[c], h);
            lo[c] = a < lo[c] ? a : lo[c];
            hi[c] = b > hi[c] ? b : hi[c];
        }
    }
    __shared__ unsigned long long w_v[4][6];
    __shared__ unsigned w_bad[4];
    const unsigned n_bad = (unsigned)__popcll(__ballot(bad));
    if ((threadIdx.x & 63u) == 0u) {
        const int w = (int)(threadIdx.x >> 6);
#pragma unroll
        for (int c = 0; c < 3; c++) { w_v[w][c] = lo[c]; w_v[w][3 + c] = hi[c]; }
        w_bad[w] = n_bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) {
            unsigned long long l = w_v[0][c], h = w_v[0][3 + c];
            for (int w = 1; w < 4; w++) { l = w_v[w][c] < l ? w_v[w][c] : l; h = w_v[w][3 + c] > h ? w_v[w][3 + c] : h; }
            if (l <= h) { atomicMin(head->box + c, l); atomicMax(head->box + 3 + c, h); }      // (a workgroup of bad vertices holds the identities)
        }
        const unsigned total = w_bad[0] + w_bad[1] + w_bad[2] + w_bad[3];
        if (total) atomicAdd(&head->n_bad, total);
    }
}

__global__ __launch_bounds__(256) void k_cluster_keys(const double *__restrict__ pts, long long n, SimplifyGrid g, unsigned long long *__restrict__ keys,
                                                      unsigned *__restrict__ idx) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    unsigned long long key = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double fq = grid_floor(pts[3 * v + c], g.origin[c], g.cell[c]);
        key = (key << KEY_BITS) | ((unsigned long long)(long long)(fq - g.fqmin[c]) & KEY_MASK);     // (both are whole numbers below 2^53: exact)
    }
    keys[v] = key;
    idx[v] = (unsigned)v;
}

__global__ __launch_bounds__(256) void k_cluster_flags(const unsigned long long *__restrict__ keys, long long n, int *__restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// one lane per position of the sorted vertices; vstart holds n + 1 words
__global__ __launch_bounds__(256) void k_cluster_number(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ idx,
                                                        const int *__restrict__ flags, const int *__restrict__ rank, long long n,
                                                        int *__restrict__ vertex_cluster, unsigned long long *__restrict__ cluster_key,
                                                        int *__restrict__ vstart) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = rank[i] + flags[i] - 1;
    vertex_cluster[idx[i]] = k;
    if (flags[i]) { cluster_key[k] = keys[i]; vstart[k] = (int)i; }
    if (i == n - 1) vstart[k + 1] = (int)n;
}

// one lane per item 3t + c
__global__ __launch_bounds__(256) void k_cluster_items(const long long *__restrict__ cells, const int *__restrict__ vertex_cluster, long long n_items,
                                                       unsigned *__restrict__ item_cluster, unsigned *__restrict__ item) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_items) return;
    item_cluster[j] = (unsigned)vertex_cluster[cells[j]];
    item[j] = (unsigned)j;
}

// one lane per position of the sorted items; istart holds n_clusters + 1 words (every cluster has an item: a welded vertex is a corner)
__global__ __launch_bounds__(256) void k_item_starts(const unsigned *__restrict__ item_cluster, long long n_items, int *__restrict__ istart) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_items) return;
    const unsigned k = item_cluster[p];
    if (p == 0 || item_cluster[p - 1] != k) istart[k] = (int)p;
    if (p == n_items - 1) istart[k + 1] = (int)n_items;
}

// one lane per cluster: mean, quadric, solve, fallbacks (tests/simplify_ref.py means / quadrics / solve, operation by operation)
__global__ __launch_bounds__(256) void k_cluster_vertex(const double *__restrict__ pts, const long long *__restrict__ cells, long long n_vertices,
                                                        long long n_items, const unsigned long long *__restrict__ cluster_key,
                                                        const int *__restrict__ vstart, const unsigned *__restrict__ idx,
                                                        const int *__restrict__ istart, const unsigned *__restrict__ item, long long n_clusters,
                                                        SimplifyGrid g, double *__restrict__ verts, SimplifyHead *head) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    bool is_flat = false, fell_back = false;
    if (k < n_clusters) {
        const unsigned long long key = cluster_key[k];
        double ctr[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const long long q = g.qmin[c] + (long long)((key >> (KEY_BITS * (2 - c))) & KEY_MASK);
            ctr[c] = g.origin[c] + ((double)q + 0.5) * g.cell[c];
        }
        // the mean of the cluster's vertices about the centre, in ascending welded index
        long long v0 = vstart[k], v1 = vstart[k + 1];
        v1 = v1 < n_vertices ? v1 : n_vertices;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (long long i = v0; i < v1; i++) {
            const long long v = idx[i];
            s0 = s0 + (pts[3 * v] - ctr[0]);
            s1 = s1 + (pts[3 * v + 1] - ctr[1]);
            s2 = s2 + (pts[3 * v + 2] - ctr[2]);
        }
        const double count = (double)(v1 - v0);
        const double m0 = s0 / count, m1 = s1 / count, m2 = s2 / count;
        // the quadric: the planes of the triangles that touch the cluster, in ascending item index
        long long i0 = istart[k], i1 = istart[k + 1];
        i1 = i1 < n_items ? i1 : n_items;
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (long long p = i0; p < i1; p++) {
            const long long t = (long long)(item[p] / 3u);
            const long long ia = cells[3 * t], ib = cells[3 * t + 1], ic = cells[3 * t + 2];
            const double ax = pts[3 * ia] - ctr[0], ay = pts[3 * ia + 1] - ctr[1], az = pts[3 * ia + 2] - ctr[2];
            const double bx = pts[3 * ib] - ctr[0], by = pts[3 * ib + 1] - ctr[1], bz = pts[3 * ib + 2] - ctr[2];
            const double cx = pts[3 * ic] - ctr[0], cy = pts[3 * ic + 1] - ctr[1], cz = pts[3 * ic + 2] - ctr[2];
            const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
            const double e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
            const double nx = (e1y * e2z) - (e1z * e2y);
            const double ny = (e1z * e2x) - (e1x * e2z);
            const double nz = (e1x * e2y) - (e1y * e2x);
            const double d = (nx * ax + ny * ay) + nz * az;
            a00 = a00 + nx * nx; a01 = a01 + nx * ny; a02 = a02 + nx * nz;
            a11 = a11 + ny * ny; a12 = a12 + ny * nz; a22 = a22 + nz * nz;
            b0 = b0 + nx * d; b1 = b1 + ny * d; b2 = b2 + nz * d;
        }
        // (A + reg w I) y = b - A m, x = m + y
        const double w = (a00 + a11) + a22;
        const double lam = g.reg * w;
        const double g0 = b0 - ((a00 * m0 + a01 * m1) + a02 * m2);
        const double g1 = b1 - ((a01 * m0 + a11 * m1) + a12 * m2);
        const double g2 = b2 - ((a02 * m0 + a12 * m1) + a22 * m2);
        const double d00 = a00 + lam;
        const double d11 = a11 + lam;
        const double d22 = a22 + lam;
        const double c00 = (d11 * d22) - (a12 * a12);
        const double c01 = (a02 * a12) - (a01 * d22);
        const double c02 = (a01 * a12) - (a02 * d11);
        const double c11 = (d00 * d22) - (a02 * a02);
        const double c12 = (a01 * a02) - (d00 * a12);
        const double c22 = (d00 * d11) - (a01 * a01);
        const double det = (d00 * c00 + a01 * c01) + a02 * c02;
        const double y0 = ((c00 * g0 + c01 * g1) + c02 * g2) / det;
        const double y1 = ((c01 * g0 + c11 * g1) + c12 * g2) / det;
        const double y2 = ((c02 * g0 + c12 * g1) + c22 * g2) / det;
        double x0 = m0 + y0, x1 = m1 + y1, x2 = m2 + y2;
        is_flat = w == 0.0;
        const bool inside = isfinite(x0) && isfinite(x1) && isfinite(x2) && fabs(x0) <= g.cell[0] * 0.5 && fabs(x1) <= g.cell[1] * 0.5 &&
                            fabs(x2) <= g.cell[2] * 0.5;
        fell_back = !is_flat && !inside;
        if (is_flat || fell_back) { x0 = m0; x1 = m1; x2 = m2; }
        verts[3 * k] = ctr[0] + x0;
        verts[3 * k + 1] = ctr[1] + x1;
        verts[3 * k + 2] = ctr[2] + x2;
    }
    __shared__ unsigned long long w_n[4];
    const unsigned long long n = ((unsigned long long)__popcll(__ballot(is_flat)) << 32) | (unsigned long long)__popcll(__ballot(fell_back));
    if ((threadIdx.x & 63u) == 0u) w_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long total = w_n[0] + w_n[1] + w_n[2] + w_n[3];
        if (total) atomicAdd(&head->counters, total);
    }
}

__global__ __launch_bounds__(256) void k_cluster_live(const long long *__restrict__ cells, const int *__restrict__ vertex_cluster, long long n_tris,
                                                      int *__restrict__ flags) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tris) return;
    const int a = vertex_cluster[cells[3 * t]], b = vertex_cluster[cells[3 * t + 1]], c = vertex_cluster[cells[3 * t + 2]];
    flags[t] = (a != b && b != c && a != c) ? 1 : 0;
}

// one lane per double of the source triangles: a survivor's nine doubles go to 9 * pos[triangle], contiguous across the wave
__global__ __launch_bounds__(256) void k_cluster_emit(const long long *__restrict__ cells, const int *__restrict__ vertex_cluster,
                                                      const double *__restrict__ verts, const int *__restrict__ flags, const int *__restrict__ pos,
                                                      long long n_doubles, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_doubles) return;
    const long long t = i / 9;
    if (!flags[t]) return;
    const int r = (int)(i - 9 * t), corner = r / 3;
    out[9ll * pos[t] + r] = verts[3ll * vertex_cluster[cells[3 * t + corner]] + (r - 3 * corner)];
}

int simplify_device(hipStream_t st, const double *d_points, const long long *d_cells, long long n_vertices, long long n_tris,
                    const double *origin, const double *cell, double reg, DevBuf *out, sdf_simplify_stats *stats, double kernel_ms[4]) {
    static const char who[] = "sdf_mesh_simplify: ";
    const long long n_items = 3 * n_tris;
    if (n_tris < 1 || n_vertices < 1 || n_items >= (1ll << 31) || n_vertices >= (1ll << 31))
        return fail(std::string(who) + "the triangle or vertex count is out of range");
    SimplifyGrid g = {};
    for (int c = 0; c < 3; c++) { g.origin[c] = origin[c]; g.cell[c] = cell[c]; }
    g.reg = reg;
    SimplifyHead h_head = {};
    size_t tmp_bytes = 0, need = 0;
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned *)nullptr,
                                                      (unsigned *)nullptr, (int)n_vertices, 0, 64, st));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(nullptr, need, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr,
                                                      (int)n_items, 0, 32, st));
    tmp_bytes = need > tmp_bytes ? need : tmp_bytes;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n_vertices > n_tris ? n_vertices : n_tris, &tmp_bytes));
    const size_t nv = (size_t)n_vertices, ni = (size_t)n_items, nt = (size_t)n_tris;
    SimplifyHead *head;
    unsigned long long *keys0, *keys1, *cluster_key;
    unsigned *idx0, *idx1, *icl0, *icl1, *item0, *item1;
    int *flags, *rank, *vertex_cluster, *vstart, *istart, *tflags, *tpos;
    double *verts;
    unsigned char *tmp;
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    scratch.part(&head, 1);
    scratch.part(&keys0, nv); scratch.part(&keys1, nv);
    scratch.part(&idx0, nv); scratch.part(&idx1, nv);
    scratch.part(&flags, nv); scratch.part(&rank, nv); scratch.part(&vertex_cluster, nv);
    scratch.part(&cluster_key, nv);
    scratch.part(&vstart, nv + 1); scratch.part(&istart, nv + 1);
    scratch.part(&icl0, ni); scratch.part(&icl1, ni); scratch.part(&item0, ni); scratch.part(&item1, ni);
    scratch.part(&verts, 3 * nv);
    scratch.part(&tflags, nt); scratch.part(&tpos, nt);
    scratch.part(&tmp, tmp_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());

    EventTimer t_keys, t_items, t_vertex, t_emit;
    // ---- the box of the grid coordinates; the refusals that need it ----
    HIPCHK_MSG(who, t_keys.start(st));
    hipLaunchKernelGGL(k_cluster_head_init, dim3(1), dim3(64), 0, st, head);
    HIPCHK_MSG(who, hipGetLastError());
    HIPCHK_MSG(who, launch_rows(k_cluster_box, n_vertices, st, d_points, n_vertices, g, head));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(SimplifyHead), hipMemcpyDeviceToHost, st));
    HIPCHK_MSG(who, stream_wait(st));
    if (h_head.n_bad) return fail(std::string(who) + std::to_string(h_head.n_bad) + " vertices are not finite");
    int x_bits = KEY_BITS;
    for (int c = 0; c < 3; c++) {
        double lo, hi;
        const unsigned long long ul = box_bits(h_head.box[c]), uh = box_bits(h_head.box[3 + c]);
        memcpy(&lo, &ul, 8); memcpy(&hi, &uh, 8);
        if (!(std::fabs(lo) < 9007199254740992.0 && std::fabs(hi) < 9007199254740992.0) || !(hi - lo < (double)(1ll << KEY_BITS)))
            return fail(std::string(who) + "the clusters span 2^21 or more cells on an axis (the cell is too small for this mesh)");
        g.fqmin[c] = lo;
        g.qmin[c] = (long long)lo;
        if (c == 0) x_bits = bits_for((long long)(hi - lo) + 1);
    }
    // ---- the clusters, numbered by ascending key ----
    HIPCHK_MSG(who, launch_rows(k_cluster_keys, n_vertices, st, d_points, n_vertices, g, keys0, idx0));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys0, keys1, idx0, idx1, (int)n_vertices, 0, 2 * KEY_BITS + x_bits, st));
    HIPCHK_MSG(who, launch_rows(k_cluster_flags, n_vertices, st, keys1, n_vertices, flags));
    long long n_clusters = 0, kept = 0;
    if (number_flags(who, "cluster flags", st, flags, rank, n_vertices, tmp, tmp_bytes, &n_clusters)) return 1;
    if (n_clusters < 1) return fail(std::string(who) + "the scan of the cluster flags is inconsistent");
    HIPCHK_MSG(who, launch_rows(k_cluster_number, n_vertices, st, keys1, idx1, flags, rank, n_vertices, vertex_cluster, cluster_key, vstart));
    HIPCHK_MSG(who, t_keys.stop(st));
    // ---- the items of every cluster, in ascending item index ----
    HIPCHK_MSG(who, t_items.start(st));
    HIPCHK_MSG(who, hipMemsetAsync(istart, 0, (size_t)(n_clusters + 1) * 4, st));
    HIPCHK_MSG(who, launch_rows(k_cluster_items, n_items, st, d_cells, vertex_cluster, n_items, icl0, item0));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, icl0, icl1, item0, item1, (int)n_items, 0, bits_for(n_clusters), st));
    HIPCHK_MSG(who, launch_rows(k_item_starts, n_items, st, icl1, n_items, istart));
    HIPCHK_MSG(who, t_items.stop(st));
    // ---- one representative per cluster ----
    HIPCHK_MSG(who, t_vertex.start(st));
    HIPCHK_MSG(who, launch_rows(k_cluster_vertex, n_clusters, st, d_points, d_cells, n_vertices, n_items, cluster_key, vstart, idx1, istart, item1,
                                n_clusters, g, verts, head));
    HIPCHK_MSG(who, t_vertex.stop(st));
    // ---- the survivors ----
    HIPCHK_MSG(who, t_emit.start(st));
    HIPCHK_MSG(who, launch_rows(k_cluster_live, n_tris, st, d_cells, vertex_cluster, n_tris, tflags));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(SimplifyHead), hipMemcpyDeviceToHost, st));    // (lands behind number_flags' wait)
    if (number_flags(who, "live flags", st, tflags, tpos, n_tris, tmp, tmp_bytes, &kept)) return 1;
    if (kept > 0) {
        if (out->ensure((size_t)kept * 72)) return 1;
        HIPCHK_MSG(who, launch_rows(k_cluster_emit, 9 * n_tris, st, d_cells, vertex_cluster, verts, tflags, tpos, 9 * n_tris, out->p));
    }
    HIPCHK_MSG(who, t_emit.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, t_keys.ms(&kernel_ms[0]));
    HIPCHK_MSG(who, t_items.ms(&kernel_ms[1]));
    HIPCHK_MSG(who, t_vertex.ms(&kernel_ms[2]));
    HIPCHK_MSG(who, t_emit.ms(&kernel_ms[3]));
    stats->clusters = (int64_t)n_clusters;
    stats->triangles_in = (int64_t)n_tris;
    stats->triangles_out = (int64_t)kept;
    stats->collapsed = (int64_t)(n_tris - kept);
    stats->flat = (int64_t)(h_head.counters >> 32);
    stats->mean_fallback = (int64_t)(h_head.counters & 0xffffffffull);
    stats->kernel_ms = kernel_ms[0] + kernel_ms[1] + kernel_ms[2] + kernel_ms[3];
    return 0;
}

}  // namespace sdfk
