// sdf_simplify.hip -- a welded mesh simplified on the device (sdf_mesh_simplify, ABI 17): Rossignac-Borrel
// vertex clustering on a uniform grid with one representative per cluster placed by a quadric error function (Lindstrom's
// out-of-core simplification).  tests/simplify_ref.py is the definition, and what is written here copies its float64 operations one
// by one, in its order: this unit is built with -ffp-contract=off, like sdf_measure.hip, and nothing below is fused.
//
// The passes.  k_cluster_box: one lane per welded vertex, the floor of its grid coordinates as ordered integer keys (box_key of
// sdf_block.h), reduced across the workgroup, at most six integer atomics per workgroup; it also counts the vertices that are not finite.
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
//
// To a tolerance (sdf_mesh_simplify_adaptive; DESIGN.md section 4p, tests/adaptive_ref.py is the definition): the passes above are
// one LEVEL (cluster_level), run on the grids of cell x 2^L from the coarsest down in the same scratch.  k_cluster_vertex<true> walks
// its items a second time for the error of the representative it settled on -- the sum of the squared residuals in the items' planes,
// sequential like the quadric -- and flags the cluster accepted when err <= tolerance^2 x w.  k_adaptive_choose, one lane per vertex,
// lets a vertex that has not chosen yet take the level's cluster if that is accepted: its id, its position, and the cluster is marked
// used; k_adaptive_count counts the used clusters and their flags; both add one integer atomic per wave.  k_adaptive_live /
// k_adaptive_emit are k_cluster_live / k_cluster_emit keyed by the chosen ids, reading the position per vertex.  On a coarse level a
// lane walks thousands of items, twice: profiles/adaptive01_tolerance.md has what that costs.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <cmath>
#include <string>

#include "sdf_block.h"
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
    wave_box_min_max(lo, hi);
    // n_bad keeps its own lines: block_count next to block_box_merge would be a second barrier.  The waves' counts are published by
    // the one barrier inside block_box_merge
    __shared__ unsigned w_bad[4];
    const unsigned n_bad = wave_count(bad);
    if ((threadIdx.x & 63u) == 0u) w_bad[threadIdx.x >> 6] = n_bad;
    block_box_merge(lo, hi, head->box);                                // (a workgroup of bad vertices holds the identities)
    if (threadIdx.x == 0) {
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

// what the adaptive path asks of k_cluster_vertex on top of the representative (all zero on the uniform path)
struct ClusterAccept {
    double tol2;                                     // tolerance * tolerance
    unsigned char *cflags;                           // per cluster: ACCEPTED | IS_FLAT | FELL_BACK
    int always;                                      // level 0, or tol2 == +inf: every cluster is accepted
};
constexpr unsigned char ACCEPTED = 1, IS_FLAT = 2, FELL_BACK = 4;

// the plane of item's triangle t about the centre of the item's cluster: n = e1 x e2 and d = n . a' (tests/simplify_ref.py quadrics)
__device__ __forceinline__ void item_plane(const double *__restrict__ pts, const long long *__restrict__ cells, long long t, const double ctr[3],
                                           double &nx, double &ny, double &nz, double &d) {
    const long long ia = cells[3 * t], ib = cells[3 * t + 1], ic = cells[3 * t + 2];
    const double ax = pts[3 * ia] - ctr[0], ay = pts[3 * ia + 1] - ctr[1], az = pts[3 * ia + 2] - ctr[2];
    const double bx = pts[3 * ib] - ctr[0], by = pts[3 * ib + 1] - ctr[1], bz = pts[3 * ib + 2] - ctr[2];
    const double cx = pts[3 * ic] - ctr[0], cy = pts[3 * ic + 1] - ctr[1], cz = pts[3 * ic + 2] - ctr[2];
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const double e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    nx = (e1y * e2z) - (e1z * e2y);
    ny = (e1z * e2x) - (e1x * e2z);
    nz = (e1x * e2y) - (e1y * e2x);
    d = (nx * ax + ny * ay) + nz * az;
}

// one lane per cluster: mean, quadric, solve, fallbacks (tests/simplify_ref.py means / quadrics / solve, operation by operation).
// ADAPTIVE (tests/adaptive_ref.py errors / level): the lane walks its items a second time for the error of the representative it
// settled on, and writes the cluster's flags instead of counting them -- only the clusters that a vertex chooses are counted, later
template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void k_cluster_vertex(const double *__restrict__ pts, const long long *__restrict__ cells, long long n_vertices,
                                                        long long n_items, const unsigned long long *__restrict__ cluster_key,
                                                        const int *__restrict__ vstart, const unsigned *__restrict__ idx,
                                                        const int *__restrict__ istart, const unsigned *__restrict__ item, long long n_clusters,
                                                        SimplifyGrid g, double *__restrict__ verts, SimplifyHead *head, ClusterAccept acc) {
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
            double nx, ny, nz, d;
            item_plane(pts, cells, (long long)(item[p] / 3u), ctr, nx, ny, nz, d);
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
        if constexpr (ADAPTIVE) {
            // the error of the representative that is used: the squared residuals in the items' planes, in ascending item index
            double err = 0.0;
            for (long long p = i0; p < i1; p++) {
                double nx, ny, nz, d;
                item_plane(pts, cells, (long long)(item[p] / 3u), ctr, nx, ny, nz, d);
                const double r = ((nx * x0 + ny * x1) + nz * x2) - d;
                err = err + r * r;
            }
            const bool accepted = acc.always || err <= acc.tol2 * w;
            acc.cflags[k] = (unsigned char)((accepted ? ACCEPTED : 0) | (is_flat ? IS_FLAT : 0) | (fell_back ? FELL_BACK : 0));
        }
    }
    if constexpr (!ADAPTIVE) {
        const unsigned long long n[1] = {((unsigned long long)wave_count(is_flat) << 32) | wave_count(fell_back)};
        block_add_waves(n, &head->counters);                           // (packed: one atomic for both)
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

// ---- to a tolerance (sdf_mesh_simplify_adaptive; DESIGN.md section 4p, tests/adaptive_ref.py) ----
// per level: the vertices that chose it, the clusters that a vertex chose, and the flat / fallen-back ones among those
struct AdaptiveHead {
    unsigned long long n[SDF_ADAPTIVE_MAX_LEVELS + 1][4];
};

// one lane per welded vertex, run once per level from the coarsest down: a vertex that has not chosen yet takes this level if its
// cluster is accepted -- its id (the level's base + the cluster), the cluster's representative, and the cluster is marked used (every
// lane that marks a cluster stores the same byte).  One integer atomic per wave for the count
__global__ __launch_bounds__(256) void k_adaptive_choose(const int *__restrict__ vertex_cluster, const unsigned char *__restrict__ cflags,
                                                         const double *__restrict__ verts, long long n_vertices, long long base,
                                                         long long *__restrict__ id, double *__restrict__ vpos, unsigned char *__restrict__ used,
                                                         unsigned long long *counters) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    bool take = false;
    if (v < n_vertices && id[v] < 0) {
        const long long k = vertex_cluster[v];
        take = (cflags[k] & ACCEPTED) != 0;
        if (take) {
            id[v] = base + k;
            vpos[3 * v] = verts[3 * k];
            vpos[3 * v + 1] = verts[3 * k + 1];
            vpos[3 * v + 2] = verts[3 * k + 2];
            used[k] = 1;
        }
    }
    wave_add(wave_count(take), counters + 0);
}

// one lane per cluster of the level, after k_adaptive_choose: the used clusters and their flags, one integer atomic per wave each
__global__ __launch_bounds__(256) void k_adaptive_count(const unsigned char *__restrict__ cflags, const unsigned char *__restrict__ used,
                                                        long long n_clusters, unsigned long long *counters) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool u = k < n_clusters && used[k] != 0;
    const unsigned char f = u ? cflags[k] : (unsigned char)0;
    wave_add(wave_count(u), counters + 1);
    wave_add(wave_count((f & IS_FLAT) != 0), counters + 2);
    wave_add(wave_count((f & FELL_BACK) != 0), counters + 3);
}

__global__ __launch_bounds__(256) void k_adaptive_unchosen(long long *__restrict__ id, long long n_vertices) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vertices) id[v] = -1;
}

// k_cluster_live / k_cluster_emit keyed by the chosen ids, reading the positions per welded vertex
__global__ __launch_bounds__(256) void k_adaptive_live(const long long *__restrict__ cells, const long long *__restrict__ id, long long n_tris,
                                                       int *__restrict__ flags) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tris) return;
    const long long a = id[cells[3 * t]], b = id[cells[3 * t + 1]], c = id[cells[3 * t + 2]];
    flags[t] = (a != b && b != c && a != c) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_adaptive_emit(const long long *__restrict__ cells, const double *__restrict__ vpos,
                                                       const int *__restrict__ flags, const int *__restrict__ pos, long long n_doubles,
                                                       double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_doubles) return;
    const long long t = i / 9;
    if (!flags[t]) return;
    const int r = (int)(i - 9 * t), corner = r / 3;
    out[9ll * pos[t] + r] = vpos[3 * cells[3 * t + corner] + (r - 3 * corner)];
}

// ---- the drivers ----
// the scratch of the per-level passes: what one level of clustering writes, reused by the next
struct ClusterBufs {
    SimplifyHead *head;
    unsigned long long *keys0, *keys1, *cluster_key;
    unsigned *idx0, *idx1, *icl0, *icl1, *item0, *item1;
    int *flags, *rank, *vertex_cluster, *vstart, *istart;
    double *verts;
    unsigned char *tmp;
    size_t tmp_bytes;

    // what the two library sorts and the scan of max(n_vertices, n_tris) flags need as temporary storage
    hipError_t size_tmp(hipStream_t st, long long n_vertices, long long n_items, long long n_tris) {
        size_t need = 0;
        tmp_bytes = 0;
        hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                                          (unsigned *)nullptr, (unsigned *)nullptr, (int)n_vertices, 0, 64, st);
        if (e != hipSuccess) return e;
        e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr,
                                               (int)n_items, 0, 32, st);
        if (e != hipSuccess) return e;
        tmp_bytes = need > tmp_bytes ? need : tmp_bytes;
        return scan_tmp_bytes(st, n_vertices > n_tris ? n_vertices : n_tris, &tmp_bytes);
    }
    // the parts up to the representatives; the caller names its own parts next and `tmp` last
    void parts(Scratch &scratch, size_t nv, size_t ni) {
        scratch.part(&head, 1);
        scratch.part(&keys0, nv); scratch.part(&keys1, nv);
        scratch.part(&idx0, nv); scratch.part(&idx1, nv);
        scratch.part(&flags, nv); scratch.part(&rank, nv); scratch.part(&vertex_cluster, nv);
        scratch.part(&cluster_key, nv);
        scratch.part(&vstart, nv + 1); scratch.part(&istart, nv + 1);
        scratch.part(&icl0, ni); scratch.part(&icl1, ni); scratch.part(&item0, ni); scratch.part(&item1, ni);
        scratch.part(&verts, 3 * nv);
    }
};

// One level of clustering on the grid g (origin, cell, reg set; fqmin and qmin are filled in here): box and refusals, keys, library
// sort, numbering, items, item sort, one lane per cluster.  Leaves vertex_cluster, verts and -- with acc.cflags -- the clusters' flags
// in b, the box it read in *h_box and the number of clusters in *n_clusters.  t3 (or nullptr): the timers of keys and numbering, the items, k_cluster_vertex
static int cluster_level(const char *who, hipStream_t st, const double *d_points, const long long *d_cells, long long n_vertices, long long n_items,
                         SimplifyGrid &g, const ClusterBufs &b, const ClusterAccept &acc, EventTimer *t3, SimplifyHead *h_box,
                         long long *n_clusters_out) {
    SimplifyHead &h_head = *h_box;                                     // (the caller's, declared before its Scratch: see there)
    size_t tmp_bytes = b.tmp_bytes;                                    // (the library's calls take it by reference)
    // ---- the box of the grid coordinates; the refusals that need it ----
    if (t3) HIPCHK_MSG(who, t3[0].start(st));
    hipLaunchKernelGGL(k_cluster_head_init, dim3(1), dim3(64), 0, st, b.head);
    HIPCHK_MSG(who, hipGetLastError());
    HIPCHK_MSG(who, launch_rows(k_cluster_box, n_vertices, st, d_points, n_vertices, g, b.head));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, b.head, sizeof(SimplifyHead), hipMemcpyDeviceToHost, st));
    HIPCHK_MSG(who, stream_wait(st));
    if (h_head.n_bad) return fail(std::string(who) + std::to_string(h_head.n_bad) + " vertices are not finite");
    int x_bits = KEY_BITS;
    for (int c = 0; c < 3; c++) {
        const double lo = box_value(h_head.box[c]), hi = box_value(h_head.box[3 + c]);
        if (!(std::fabs(lo) < 9007199254740992.0 && std::fabs(hi) < 9007199254740992.0) || !(hi - lo < (double)(1ll << KEY_BITS)))
            return fail(std::string(who) + "the clusters span 2^21 or more cells on an axis (the cell is too small for this mesh)");
        g.fqmin[c] = lo;
        g.qmin[c] = (long long)lo;
        if (c == 0) x_bits = bits_for((long long)(hi - lo) + 1);
    }
    // ---- the clusters, numbered by ascending key ----
    HIPCHK_MSG(who, launch_rows(k_cluster_keys, n_vertices, st, d_points, n_vertices, g, b.keys0, b.idx0));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(b.tmp, tmp_bytes, b.keys0, b.keys1, b.idx0, b.idx1, (int)n_vertices, 0, 2 * KEY_BITS + x_bits, st));
    HIPCHK_MSG(who, launch_rows(k_cluster_flags, n_vertices, st, b.keys1, n_vertices, b.flags));
    long long n_clusters = 0;
    if (number_flags(who, "cluster flags", st, b.flags, b.rank, n_vertices, b.tmp, tmp_bytes, &n_clusters)) return 1;
    if (n_clusters < 1) return fail(std::string(who) + "the scan of the cluster flags is inconsistent");
    HIPCHK_MSG(who, launch_rows(k_cluster_number, n_vertices, st, b.keys1, b.idx1, b.flags, b.rank, n_vertices, b.vertex_cluster, b.cluster_key, b.vstart));
    if (t3) HIPCHK_MSG(who, t3[0].stop(st));
    // ---- the items of every cluster, in ascending item index ----
    if (t3) HIPCHK_MSG(who, t3[1].start(st));
    HIPCHK_MSG(who, hipMemsetAsync(b.istart, 0, (size_t)(n_clusters + 1) * 4, st));
    HIPCHK_MSG(who, launch_rows(k_cluster_items, n_items, st, d_cells, b.vertex_cluster, n_items, b.icl0, b.item0));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(b.tmp, tmp_bytes, b.icl0, b.icl1, b.item0, b.item1, (int)n_items, 0, bits_for(n_clusters), st));
    HIPCHK_MSG(who, launch_rows(k_item_starts, n_items, st, b.icl1, n_items, b.istart));
    if (t3) HIPCHK_MSG(who, t3[1].stop(st));
    // ---- one representative per cluster ----
    if (t3) HIPCHK_MSG(who, t3[2].start(st));
    if (acc.cflags)
        HIPCHK_MSG(who, launch_rows(k_cluster_vertex<true>, n_clusters, st, d_points, d_cells, n_vertices, n_items, b.cluster_key, b.vstart, b.idx1,
                                    b.istart, b.item1, n_clusters, g, b.verts, b.head, acc));
    else
        HIPCHK_MSG(who, launch_rows(k_cluster_vertex<false>, n_clusters, st, d_points, d_cells, n_vertices, n_items, b.cluster_key, b.vstart, b.idx1,
                                    b.istart, b.item1, n_clusters, g, b.verts, b.head, acc));
    if (t3) HIPCHK_MSG(who, t3[2].stop(st));
    *n_clusters_out = n_clusters;
    return 0;
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
    ClusterBufs b = {};
    HIPCHK_MSG(who, b.size_tmp(st, n_vertices, n_items, n_tris));
    int *tflags, *tpos;
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    b.parts(scratch, (size_t)n_vertices, (size_t)n_items);
    scratch.part(&tflags, (size_t)n_tris); scratch.part(&tpos, (size_t)n_tris);
    scratch.part(&b.tmp, b.tmp_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());

    EventTimer t3[3], t_emit;
    long long n_clusters = 0, kept = 0;
    if (cluster_level(who, st, d_points, d_cells, n_vertices, n_items, g, b, ClusterAccept{}, t3, &h_head, &n_clusters)) return 1;
    // ---- the survivors ----
    HIPCHK_MSG(who, t_emit.start(st));
    HIPCHK_MSG(who, launch_rows(k_cluster_live, n_tris, st, d_cells, b.vertex_cluster, n_tris, tflags));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, b.head, sizeof(SimplifyHead), hipMemcpyDeviceToHost, st));    // (lands behind number_flags' wait)
    if (number_flags(who, "live flags", st, tflags, tpos, n_tris, b.tmp, b.tmp_bytes, &kept)) return 1;
    if (kept > 0) {
        if (out->ensure((size_t)kept * 72)) return 1;
        HIPCHK_MSG(who, launch_rows(k_cluster_emit, 9 * n_tris, st, d_cells, b.vertex_cluster, b.verts, tflags, tpos, 9 * n_tris, out->p));
    }
    HIPCHK_MSG(who, t_emit.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    for (int k = 0; k < 3; k++) HIPCHK_MSG(who, t3[k].ms(&kernel_ms[k]));
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

int simplify_adaptive_device(hipStream_t st, const double *d_points, const long long *d_cells, long long n_vertices, long long n_tris,
                             const double *origin, const double *cell, double reg, double tolerance, int levels, DevBuf *out,
                             sdf_adaptive_stats *stats, double *level_ms, double *emit_ms) {
    static const char who[] = "sdf_mesh_simplify_adaptive: ";
    const long long n_items = 3 * n_tris;
    if (n_tris < 1 || n_vertices < 1 || n_items >= (1ll << 31) || n_vertices >= (1ll << 31))
        return fail(std::string(who) + "the triangle or vertex count is out of range");
    if (levels < 0 || levels > SDF_ADAPTIVE_MAX_LEVELS || !(tolerance >= 0.0)) return fail(std::string(who) + "levels or tolerance is out of range");
    const double tol2 = tolerance * tolerance;
    AdaptiveHead h_head = {};
    SimplifyHead h_box = {};
    ClusterBufs b = {};
    HIPCHK_MSG(who, b.size_tmp(st, n_vertices, n_items, n_tris));
    const size_t nv = (size_t)n_vertices;
    AdaptiveHead *head;
    unsigned char *cflags, *used;
    long long *id;
    double *vpos;
    int *tflags, *tpos;
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    b.parts(scratch, nv, (size_t)n_items);
    scratch.part(&head, 1);
    scratch.part(&cflags, nv); scratch.part(&used, nv);                // (a level has no more clusters than there are vertices)
    scratch.part(&id, nv); scratch.part(&vpos, 3 * nv);
    scratch.part(&tflags, (size_t)n_tris); scratch.part(&tpos, (size_t)n_tris);
    scratch.part(&b.tmp, b.tmp_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());

    EventTimer t_level[SDF_ADAPTIVE_MAX_LEVELS + 1], t_emit;
    HIPCHK_MSG(who, hipMemsetAsync(head, 0, sizeof(AdaptiveHead), st));
    HIPCHK_MSG(who, launch_rows(k_adaptive_unchosen, n_vertices, st, id, n_vertices));
    long long base = 0, kept = 0;
    for (int lv = levels; lv >= 0; lv--) {                             // from the coarsest down: the first level that accepts is the coarsest
        SimplifyGrid g = {};
        for (int c = 0; c < 3; c++) { g.origin[c] = origin[c]; g.cell[c] = cell[c] * (double)(1 << lv); }
        g.reg = reg;
        ClusterAccept acc = {};
        acc.tol2 = tol2;
        acc.cflags = cflags;
        acc.always = (lv == 0 || std::isinf(tol2)) ? 1 : 0;
        long long n_clusters = 0;
        HIPCHK_MSG(who, t_level[lv].start(st));
        if (cluster_level(who, st, d_points, d_cells, n_vertices, n_items, g, b, acc, nullptr, &h_box, &n_clusters)) return 1;
        HIPCHK_MSG(who, hipMemsetAsync(used, 0, (size_t)n_clusters, st));
        HIPCHK_MSG(who, launch_rows(k_adaptive_choose, n_vertices, st, b.vertex_cluster, cflags, b.verts, n_vertices, base, id, vpos, used, head->n[lv]));
        HIPCHK_MSG(who, launch_rows(k_adaptive_count, n_clusters, st, cflags, used, n_clusters, head->n[lv]));
        HIPCHK_MSG(who, t_level[lv].stop(st));
        base += n_clusters;
    }
    // ---- the survivors ----
    HIPCHK_MSG(who, t_emit.start(st));
    HIPCHK_MSG(who, launch_rows(k_adaptive_live, n_tris, st, d_cells, id, n_tris, tflags));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(AdaptiveHead), hipMemcpyDeviceToHost, st));    // (lands behind number_flags' wait)
    if (number_flags(who, "live flags", st, tflags, tpos, n_tris, b.tmp, b.tmp_bytes, &kept)) return 1;
    if (kept > 0) {
        if (out->ensure((size_t)kept * 72)) return 1;
        HIPCHK_MSG(who, launch_rows(k_adaptive_emit, 9 * n_tris, st, d_cells, vpos, tflags, tpos, 9 * n_tris, out->p));
    }
    HIPCHK_MSG(who, t_emit.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    *stats = sdf_adaptive_stats();
    stats->kernel_ms = 0.0;
    for (int lv = 0; lv <= levels; lv++) {
        HIPCHK_MSG(who, t_level[lv].ms(&level_ms[lv]));
        stats->kernel_ms += level_ms[lv];
        stats->vertices[lv] = (int64_t)h_head.n[lv][0];
        stats->clusters_used[lv] = (int64_t)h_head.n[lv][1];
        stats->flat += (int64_t)h_head.n[lv][2];
        stats->mean_fallback += (int64_t)h_head.n[lv][3];
    }
    HIPCHK_MSG(who, t_emit.ms(emit_ms));
    stats->kernel_ms += *emit_ms;
    stats->triangles_in = (int64_t)n_tris;
    stats->triangles_out = (int64_t)kept;
    stats->collapsed = (int64_t)(n_tris - kept);
    stats->levels = (int64_t)levels;
    return 0;
}

}  // namespace sdfk
