// sdf_contour.hip -- the contours of a sampled 2-D field (sdf_contour_grid_host, sdf_contour_host; added under ABI 17; DESIGN.md
// section 4m): marching squares whose segments leave the device as closed, oriented polylines in an order that is a function of the
// grid alone.  tests/contour_ref.py is the definition and every output is reproduced bit for bit: float64, one rounding per written
// operation (-ffp-contract=off), the vertex of a grid edge always from the lower-index sample, t = (a - level) / (a - b),
// c = ca + t * (cb - ca).
//
// Samples V[nw][nx][ny], cells g = w * ncell + ix * (ny - 1) + iy, one lane per cell with the lanes along iy.
//   k_contour_count    the cell's code (its case, bit 4: the centre value is inside) and its number of segments, 0 .. 2; the cells with
//                      a non-finite corner are counted (block_count of sdf_block.h).  The library scan gives the offsets.
//   k_contour_emit     per segment s: its start vertex; its successor -- the slot of the cell across the edge where s ends whose `from`
//                      is that edge, from the neighbour's code and offset -- is not stored: s writes s + 1 into pred[successor] (a
//                      zeroed array; a segment has at most one predecessor, so a plain store).  A segment without a successor (the
//                      border of the grid, a non-finite neighbour) leaves (g << 2 | to) + 1 in tail[s], else 0.
// Linking is pointer jumping over the PREDECESSORS, integers only, `rounds` = ceil(log2(n_segments)) launches per phase, the count
// from the host, two buffers of (int, int) that swap roles -- a round reads one and writes the other:
//   (a) k_link_init / k_link_min: (m, b) = (the smallest index among the 2^r segments from s backwards, the segment 2^r steps back);
//       a segment without a predecessor points at itself.  Afterwards m is a closed loop's smallest index and b an open chain's head.
//   (b) k_link_leader picks the leader (the head if pred[b] is empty, else m), flags it, and cuts the list there: (d, b) = (0, s) for a
//       leader, (1, pred) for the others; k_link_rank doubles d, which ends as the segment's position in its contour.
//   (c) the flags are numbered (ascending leader index = the order of the contours); k_contour_lengths has the last segment of every
//       contour write its number of points; a second scan gives the offsets.
//   (d) k_contour_scatter writes every start vertex to offsets[contour] + d, the end vertex of an open chain's last segment behind
//       it, and -- the leader's lane -- closed, layer (a binary search over the layers' first offsets) and the 64-bit offset.
//   k_contour_area     one lane per contour walks its points in order: the shoelace sum is the definition's, left to right (eight
//                      loads in flight, their terms added in order; a contour of 10^6 points takes one lane 39 ms).
// The tape entry fills V through sdf_eval_points, from points that k_contour_points writes in slabs of at most 2^24.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "sdf_block.h"
#include "sdf_contour.h"
#include "sdf_internal.h"
#include "sdf_prims.h"

using namespace sdfk;

namespace {

struct ContourHead {
    unsigned long long nonfinite;
};

struct CGrid {
    int nw, nx, ny;                                                    // (nw * nx * ny <= 2^28: every index below fits 32 bits)
    double level;
};

// the segments of a cell from its code: n, and (from, to) per slot
__device__ __forceinline__ int code_segments(unsigned code, int f[2], int t[2]) {
    const unsigned char *r = CONTOUR_CASES[code & 15u];
    const int n = r[0];
    const bool swap = n == 2 && !(code & 16u);
    f[0] = r[1]; f[1] = r[3];
    t[0] = swap ? r[4] : r[2]; t[1] = swap ? r[2] : r[4];
    return n;
}

// the vertex on edge e of cell (ix, iy) of the layer at L
__device__ __forceinline__ void edge_vertex(const double *__restrict__ L, const double *__restrict__ X, const double *__restrict__ Y, int ny,
                                            int ix, int iy, int e, double level, double *x, double *y) {
    if (e == 0 || e == 2) {
        const int j = iy + (e == 2 ? 1 : 0);
        const double a = L[(size_t)ix * ny + j], b = L[(size_t)(ix + 1) * ny + j];
        const double t = (a - level) / (a - b);
        *x = X[ix] + t * (X[ix + 1] - X[ix]);
        *y = Y[j];
    } else {
        const int i = ix + (e == 1 ? 1 : 0);
        const double a = L[(size_t)i * ny + iy], b = L[(size_t)i * ny + iy + 1];
        const double t = (a - level) / (a - b);
        *x = X[i];
        *y = Y[iy] + t * (Y[iy + 1] - Y[iy]);
    }
}

// the points of samples [s0, s0 + m) of the grid, dim doubles each: (X[ix], Y[iy]) and, dim 3, W[w]
__global__ __launch_bounds__(256) void k_contour_points(const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ W,
                                                        int nx, int ny, int dim, long long s0, int m, double *__restrict__ pts) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= m) return;
    const long long s = s0 + i;
    const int iy = (int)(s % ny), ix = (int)((s / ny) % nx), w = (int)(s / ((long long)nx * ny));
    pts[(size_t)i * dim] = X[ix];
    pts[(size_t)i * dim + 1] = Y[iy];
    if (dim == 3) pts[(size_t)i * dim + 2] = W[w];
}

__global__ __launch_bounds__(256) void k_contour_count(const double *__restrict__ V, const CGrid gr, int n_cells, int *__restrict__ cnt,
                                                       unsigned char *__restrict__ code, ContourHead *head) {
    const int g = (int)(blockIdx.x * 256u + threadIdx.x);
    bool bad[1] = {false};
    if (g < n_cells) {
        const int cy = gr.ny - 1, ncell = (gr.nx - 1) * cy;
        const int w = g / ncell, c = g - w * ncell, ix = c / cy, iy = c - ix * cy;
        const double *L = V + (size_t)w * gr.nx * gr.ny;
        const double c0 = L[(size_t)ix * gr.ny + iy], c3 = L[(size_t)ix * gr.ny + iy + 1];
        const double c1 = L[(size_t)(ix + 1) * gr.ny + iy], c2 = L[(size_t)(ix + 1) * gr.ny + iy + 1];
        const bool finite = std::isfinite(c0) && std::isfinite(c1) && std::isfinite(c2) && std::isfinite(c3);
        const double centre = ((c0 + c1) + (c3 + c2)) * 0.25;
        unsigned k = (c0 < gr.level ? 1u : 0u) | (c1 < gr.level ? 2u : 0u) | (c2 < gr.level ? 4u : 0u) | (c3 < gr.level ? 8u : 0u);
        k = finite ? (k | (centre < gr.level ? 16u : 0u)) : 0u;
        bad[0] = !finite;
        code[g] = (unsigned char)k;
        cnt[g] = CONTOUR_CASES[k & 15u][0];
    }
    block_count(bad, &head->nonfinite);
}

// pred: n_seg ints, zeroed; start: n_seg x 2 doubles; tail: n_seg
__global__ __launch_bounds__(256) void k_contour_emit(const double *__restrict__ V, const double *__restrict__ X, const double *__restrict__ Y,
                                                      const CGrid gr, int n_cells, const unsigned char *__restrict__ code,
                                                      const int *__restrict__ off, int n_seg, double *__restrict__ start,
                                                      int *__restrict__ pred, unsigned *__restrict__ tail) {
    const int g = (int)(blockIdx.x * 256u + threadIdx.x);
    if (g >= n_cells) return;
    int f[2], t[2];
    const int n = code_segments(code[g], f, t);
    if (n == 0) return;
    const int cy = gr.ny - 1, ncell = (gr.nx - 1) * cy;
    const int w = g / ncell, c = g - w * ncell, ix = c / cy, iy = c - ix * cy;
    const double *L = V + (size_t)w * gr.nx * gr.ny;
    for (int k = 0; k < n; k++) {
        const int s = off[g] + k;
        if (s < 0 || s >= n_seg) return;                               // (an offset the scan did not write: nothing out of bounds)
        double x, y;
        edge_vertex(L, X, Y, gr.ny, ix, iy, f[k], gr.level, &x, &y);
        start[2 * (size_t)s] = x;
        start[2 * (size_t)s + 1] = y;
        const int e = t[k];
        const int jx = ix + (e == 1 ? 1 : (e == 3 ? -1 : 0)), jy = iy + (e == 2 ? 1 : (e == 0 ? -1 : 0));
        int next = -1;
        if (jx >= 0 && jx < gr.nx - 1 && jy >= 0 && jy < cy) {
            const int h = w * ncell + jx * cy + jy;
            int f2[2], t2[2];
            const int n2 = code_segments(code[h], f2, t2);
            const int want = (e + 2) & 3;
            for (int k2 = 0; k2 < n2; k2++) if (f2[k2] == want) next = off[h] + k2;
        }
        if (next >= 0 && next < n_seg) pred[next] = s + 1;
        tail[s] = next >= 0 ? 0u : (((unsigned)g << 2) | (unsigned)e) + 1u;
    }
}

__global__ __launch_bounds__(256) void k_link_init(const int *__restrict__ pred, int n, int2 *__restrict__ out) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= n) return;
    const int p = pred[s];
    out[s] = make_int2(s, p ? p - 1 : s);
}

__global__ __launch_bounds__(256) void k_link_min(const int2 *__restrict__ in, int n, int2 *__restrict__ out) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= n) return;
    const int2 a = in[s], q = in[a.y];
    out[s] = make_int2(a.x < q.x ? a.x : q.x, q.y);
}

__global__ __launch_bounds__(256) void k_link_leader(const int2 *__restrict__ in, const int *__restrict__ pred, int n, int *__restrict__ leader,
                                                     int *__restrict__ flag, int2 *__restrict__ out) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= n) return;
    const int2 a = in[s];
    const int ld = pred[a.y] == 0 ? a.y : a.x;                         // an open chain's head, a closed loop's smallest index
    leader[s] = ld;
    flag[s] = ld == s ? 1 : 0;
    out[s] = ld == s ? make_int2(0, s) : make_int2(1, pred[s] - 1);    // (not a leader: not a head, so it has a predecessor)
}

__global__ __launch_bounds__(256) void k_link_rank(const int2 *__restrict__ in, int n, int2 *__restrict__ out) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= n) return;
    const int2 a = in[s], q = in[a.y];
    out[s] = make_int2(a.x + q.x, q.y);
}

// the last segment of every contour writes the contour's number of points
__global__ __launch_bounds__(256) void k_contour_lengths(const int2 *__restrict__ rank, const int *__restrict__ leader, const int *__restrict__ pos,
                                                         const int *__restrict__ pred, const unsigned *__restrict__ tail, int n, int n_contours,
                                                         int *__restrict__ npts) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= n) return;
    const int ld = leader[s], c = pos[ld];
    const bool open = pred[ld] == 0;
    const bool last = open ? tail[s] != 0u : pred[ld] - 1 == s;
    if (last && c >= 0 && c < n_contours) npts[c] = rank[s].x + 1 + (open ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_contour_scatter(const double *__restrict__ V, const double *__restrict__ X, const double *__restrict__ Y,
                                                         const CGrid gr, const int *__restrict__ off, const double *__restrict__ start,
                                                         const int2 *__restrict__ rank, const int *__restrict__ leader, const int *__restrict__ pos,
                                                         const int *__restrict__ pred, const unsigned *__restrict__ tail,
                                                         const int *__restrict__ ofs, int n, int n_contours, long long n_points,
                                                         double *__restrict__ points, long long *__restrict__ offsets,
                                                         unsigned char *__restrict__ closed, int *__restrict__ layer) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= n) return;
    const int ld = leader[s], c = pos[ld];
    if (c < 0 || c >= n_contours) return;
    const long long p = (long long)ofs[c] + rank[s].x;
    const int cy = gr.ny - 1, ncell = (gr.nx - 1) * cy;
    if (p >= 0 && p < n_points) {
        points[2 * p] = start[2 * (size_t)s];
        points[2 * p + 1] = start[2 * (size_t)s + 1];
    }
    const unsigned tl = tail[s];
    if (tl != 0u && p + 1 >= 0 && p + 1 < n_points) {                  // the end of an open chain
        const int g = (int)((tl - 1u) >> 2), e = (int)((tl - 1u) & 3u);
        const int w = g / ncell, cc = g - w * ncell, ix = cc / cy, iy = cc - ix * cy;
        double x, y;
        edge_vertex(V + (size_t)w * gr.nx * gr.ny, X, Y, gr.ny, ix, iy, e, gr.level, &x, &y);
        points[2 * (p + 1)] = x;
        points[2 * (p + 1) + 1] = y;
    }
    if (ld == s) {
        int lo = 0, hi = gr.nw - 1;                                    // the last layer whose first offset is <= s
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[(size_t)mid * ncell] <= s) lo = mid; else hi = mid - 1;
        }
        layer[c] = lo;
        closed[c] = pred[s] != 0 ? 1 : 0;
        offsets[c] = ofs[c];
        if (c == n_contours - 1) offsets[n_contours] = n_points;
    }
}

__global__ __launch_bounds__(256) void k_contour_area(const double *__restrict__ points, const long long *__restrict__ offsets,
                                                      const unsigned char *__restrict__ closed, int n_contours, double *__restrict__ area) {
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    if (c >= n_contours) return;
    double acc = 0.0;
    if (closed[c]) {
        const long long p0 = offsets[c], p1 = offsets[c + 1];
        const double2 *P = (const double2 *)points;                    // (16-byte aligned: the block's first part)
        const double2 first = P[p0];
        double x = first.x, y = first.y;
        long long p = p0;
        for (; p + 8 < p1; p += 8) {                                   // eight loads in flight, then their terms IN ORDER
            double2 q[8];
#pragma unroll
            for (int k = 0; k < 8; k++) q[k] = P[p + 1 + k];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                acc = acc + (x * q[k].y - q[k].x * y);
                x = q[k].x; y = q[k].y;
            }
        }
        for (; p < p1; p++) {
            const double2 q = p + 1 == p1 ? first : P[p + 1];
            acc = acc + (x * q.y - q.x * y);
            x = q.x; y = q.y;
        }
        acc = 0.5 * acc;
    }
    area[c] = acc;
}

int rounds_for(long long n) { int r = 0; while ((1ll << r) < n) r += 1; return r; }

thread_local double g_contour_ms[4] = {0.0, 0.0, 0.0, 0.0};            // sampling, count + emit, linking, area

}  // namespace

struct sdf_contours {
    sdf_ctx *ctx = nullptr;
    DevBlock block;                                                    // points, offsets, area, layer, closed
    long long n_points = 0, n_contours = 0;
    size_t o_offsets = 0, o_area = 0, o_layer = 0, o_closed = 0;
};

namespace {

// What both entry points share.  t == nullptr: the samples come from h_values; else they are taken on the device, and copied to
// h_values_out unless that is NULL.  The arguments have been checked.
int contour_run(const char *who, sdf_ctx *c, sdf_tape *t, int dim, const double *h_values, double *h_values_out, const double *X, int nx,
                const double *Y, int ny, const double *W, int nw, double level, sdf_contours **out, sdf_contour_counts *counts) {
    HIPCHK_MSG(who, set_device(c->device));
    hipStream_t st = c->stream;
    const CGrid gr = {nw, nx, ny, level};
    const long long n_samples = (long long)nw * nx * ny, n_cells = (long long)nw * (nx - 1) * (ny - 1);
    const long long slab = n_samples < (1ll << 24) ? n_samples : (1ll << 24);
    sdf_contours *res = new sdf_contours();
    struct Guard { sdf_contours *r; ~Guard() { delete r; } } guard{res};  // (its block goes back with it)
    res->ctx = c;
    *counts = sdf_contour_counts();
    for (int k = 0; k < 4; k++) g_contour_ms[k] = 0.0;

    // ---- stage 1: what is sized by the grid ----
    size_t tmp_bytes = 0;
    HIPCHK_MSG(who, scan_tmp_bytes(st, 2 * n_cells, &tmp_bytes));      // (the segments and the contours are no more than that)
    double *V, *dX, *dY, *dW, *pts;
    int *cnt, *off;
    unsigned char *code, *tmp;
    ContourHead *head;
    Scratch grid_scratch(st);
    grid_scratch.part(&head, 1);
    grid_scratch.part(&V, (size_t)n_samples);
    grid_scratch.part(&dX, (size_t)nx); grid_scratch.part(&dY, (size_t)ny); grid_scratch.part(&dW, (size_t)nw);
    grid_scratch.part(&pts, t ? (size_t)slab * dim : 1);
    grid_scratch.part(&cnt, (size_t)n_cells); grid_scratch.part(&off, (size_t)n_cells);
    grid_scratch.part(&code, (size_t)n_cells);
    grid_scratch.part(&tmp, tmp_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(grid_scratch.bytes) + "): ", grid_scratch.alloc());
    HIPCHK_MSG(who, hipMemcpyAsync(dX, X, (size_t)nx * 8, hipMemcpyHostToDevice, st));
    HIPCHK_MSG(who, hipMemcpyAsync(dY, Y, (size_t)ny * 8, hipMemcpyHostToDevice, st));
    EventTimer t_sample, t_cells, t_link, t_area;
    if (t) {
        if (dim == 3) HIPCHK_MSG(who, hipMemcpyAsync(dW, W, (size_t)nw * 8, hipMemcpyHostToDevice, st));
        HIPCHK_MSG(who, t_sample.start(st));
        for (long long s0 = 0; s0 < n_samples; s0 += slab) {
            const long long m = n_samples - s0 < slab ? n_samples - s0 : slab;
            HIPCHK_MSG(who, launch_rows(k_contour_points, m, st, dX, dY, dW, nx, ny, dim, s0, (int)m, pts));
            if (sdf_eval_points(t, pts, m, dim, V + s0, SDF_PRECISION_F64)) return 1;
        }
        HIPCHK_MSG(who, t_sample.stop(st));
        if (h_values_out) HIPCHK_MSG(who, hipMemcpyAsync(h_values_out, V, (size_t)n_samples * 8, hipMemcpyDeviceToHost, st));
    } else {
        HIPCHK_MSG(who, hipMemcpyAsync(V, h_values, (size_t)n_samples * 8, hipMemcpyHostToDevice, st));
    }

    // ---- the cells: codes, counts, offsets ----
    ContourHead h_head = {};
    HIPCHK_MSG(who, t_cells.start(st));
    HIPCHK_MSG(who, hipMemsetAsync(head, 0, sizeof(ContourHead), st));
    HIPCHK_MSG(who, launch_rows(k_contour_count, n_cells, st, V, gr, (int)n_cells, cnt, code, head));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(ContourHead), hipMemcpyDeviceToHost, st));       // (lands behind the scan's wait)
    long long n_seg = 0;
    if (number_counts(who, "segment counts", st, cnt, off, n_cells, 2 * n_cells, tmp, tmp_bytes, &n_seg)) return 1;
    counts->n_segments = n_seg;
    counts->nonfinite_cells = (int64_t)h_head.nonfinite;
    const int rounds = rounds_for(n_seg);
    counts->rounds = rounds;

    long long n_contours = 0, n_points = 0;
    if (n_seg > 0) {
        // ---- stage 2: what is sized by the segments ----
        double *start;
        int *pred, *leader, *flag, *pos, *npts, *ofs;
        unsigned *tail;
        int2 *ping, *pong;
        Scratch seg_scratch(st);
        const size_t ns = (size_t)n_seg;
        seg_scratch.part(&start, 2 * ns);
        seg_scratch.part(&pred, ns); seg_scratch.part(&tail, ns);
        seg_scratch.part(&ping, ns); seg_scratch.part(&pong, ns);
        seg_scratch.part(&leader, ns); seg_scratch.part(&flag, ns); seg_scratch.part(&pos, ns);
        seg_scratch.part(&npts, ns); seg_scratch.part(&ofs, ns);
        HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(seg_scratch.bytes) + "): ", seg_scratch.alloc());
        HIPCHK_MSG(who, hipMemsetAsync(pred, 0, ns * 4, st));
        HIPCHK_MSG(who, launch_rows(k_contour_emit, n_cells, st, V, dX, dY, gr, (int)n_cells, code, off, (int)n_seg, start, pred, tail));
        HIPCHK_MSG(who, t_cells.stop(st));

        // ---- (a) leaders, (b) positions ----
        HIPCHK_MSG(who, t_link.start(st));
        int2 *in = ping, *other = pong;
        HIPCHK_MSG(who, launch_rows(k_link_init, n_seg, st, pred, (int)n_seg, in));
        for (int r = 0; r < rounds; r++) {
            HIPCHK_MSG(who, launch_rows(k_link_min, n_seg, st, in, (int)n_seg, other));
            int2 *x = in; in = other; other = x;
        }
        HIPCHK_MSG(who, launch_rows(k_link_leader, n_seg, st, in, pred, (int)n_seg, leader, flag, other));
        { int2 *x = in; in = other; other = x; }
        for (int r = 0; r < rounds; r++) {
            HIPCHK_MSG(who, launch_rows(k_link_rank, n_seg, st, in, (int)n_seg, other));
            int2 *x = in; in = other; other = x;
        }
        const int2 *rank = in;
        // ---- (c) the contours numbered, their lengths, their offsets ----
        if (number_flags(who, "leader flags", st, flag, pos, n_seg, tmp, tmp_bytes, &n_contours)) return 1;
        if (n_contours < 1) return fail(std::string(who) + "segments without a leader");
        HIPCHK_MSG(who, hipMemsetAsync(npts, 0, (size_t)n_contours * 4, st));
        HIPCHK_MSG(who, launch_rows(k_contour_lengths, n_seg, st, rank, leader, pos, pred, tail, (int)n_seg, (int)n_contours, npts));
        if (number_counts(who, "contour lengths", st, npts, ofs, n_contours, n_seg + n_contours, tmp, tmp_bytes, &n_points)) return 1;
        if (n_points < n_seg) return fail(std::string(who) + "the contours hold fewer points than there are segments");
        // ---- the result block; (d) the points in their final order ----
        res->o_offsets = align256((size_t)n_points * 16);
        res->o_area = res->o_offsets + align256((size_t)(n_contours + 1) * 8);
        res->o_layer = res->o_area + align256((size_t)n_contours * 8);
        res->o_closed = res->o_layer + align256((size_t)n_contours * 4);
        const size_t bytes = res->o_closed + align256((size_t)n_contours);
        HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(bytes) + "): ", res->block.alloc(bytes, st));
        char *base = res->block.as<char>();
        double *points = (double *)base, *area = (double *)(base + res->o_area);
        long long *offsets = (long long *)(base + res->o_offsets);
        int *layer = (int *)(base + res->o_layer);
        unsigned char *closed = (unsigned char *)(base + res->o_closed);
        HIPCHK_MSG(who, launch_rows(k_contour_scatter, n_seg, st, V, dX, dY, gr, off, start, rank, leader, pos, pred, tail, ofs, (int)n_seg,
                                    (int)n_contours, n_points, points, offsets, closed, layer));
        HIPCHK_MSG(who, t_link.stop(st));
        HIPCHK_MSG(who, t_area.start(st));
        HIPCHK_MSG(who, launch_rows(k_contour_area, n_contours, st, points, offsets, closed, (int)n_contours, area));
        HIPCHK_MSG(who, t_area.stop(st));
        HIPCHK_MSG(who, stream_wait(st));
        HIPCHK_MSG(who, t_link.ms(&g_contour_ms[2]));
        HIPCHK_MSG(who, t_area.ms(&g_contour_ms[3]));
    } else {
        HIPCHK_MSG(who, t_cells.stop(st));
        HIPCHK_MSG(who, stream_wait(st));
    }
    if (t) HIPCHK_MSG(who, t_sample.ms(&g_contour_ms[0]));
    HIPCHK_MSG(who, t_cells.ms(&g_contour_ms[1]));
    res->n_points = n_points; res->n_contours = n_contours;
    counts->n_points = n_points; counts->n_contours = n_contours;
    guard.r = nullptr;
    *out = res;
    return 0;
}

// 0, or 2 with the message set: what both entry points refuse about the grid
int check_grid(const char *who, const double *X, int nx, const double *Y, int ny, int nw, double level) {
    auto refuse = [&](const std::string &why) { fail(std::string(who) + why); return 2; };
    if (nx < 2 || ny < 2) return refuse("nx and ny must be 2 or more");
    if (nw < 1) return refuse("nw must be 1 or more");
    if ((long long)nw * nx * ny > (1ll << 28)) return refuse("more than 2^28 samples");
    if (!std::isfinite(level)) return refuse("the level is not finite");
    for (int k = 0; k < nx; k++) if (!std::isfinite(X[k])) return refuse("an X value is not finite");
    for (int k = 0; k < ny; k++) if (!std::isfinite(Y[k])) return refuse("a Y value is not finite");
    for (int k = 1; k < nx; k++) if (!(X[k] > X[k - 1])) return refuse("X is not strictly increasing");
    for (int k = 1; k < ny; k++) if (!(Y[k] > Y[k - 1])) return refuse("Y is not strictly increasing");
    return 0;
}

}  // namespace

extern "C" {

int sdf_contour_grid_host(sdf_ctx *c, const double *h_values, int nw, int nx, int ny, const double *X, const double *Y, double level,
                          sdf_contours **out, sdf_contour_counts *counts) {
    static const char who[] = "sdf_contour_grid_host: ";
    if (!c || !h_values || !X || !Y || !out || !counts) { fail(std::string(who) + "NULL argument"); return 2; }
    *out = nullptr;
    if (check_grid(who, X, nx, Y, ny, nw, level)) return 2;
    return contour_run(who, c, nullptr, 2, h_values, nullptr, X, nx, Y, ny, nullptr, nw, level, out, counts);
}

int sdf_contour_host(sdf_tape *t, int dim, const double *X, int nx, const double *Y, int ny, const double *W, int nw, double level,
                     double *h_values, sdf_contours **out, sdf_contour_counts *counts) {
    static const char who[] = "sdf_contour_host: ";
    auto refuse = [&](const std::string &why) { fail(std::string(who) + why); return 2; };
    if (!t || !X || !Y || !out || !counts || (dim == 3 && !W)) return refuse("NULL argument");
    *out = nullptr;
    if (dim != 2 && dim != 3) return refuse("dim must be 2 or 3");
    if (dim == 2 && nw != 1) return refuse("a 2-D model has one layer: nw must be 1");
    if (check_grid(who, X, nx, Y, ny, nw, level)) return 2;
    for (int k = 0; dim == 3 && k < nw; k++) if (!std::isfinite(W[k])) return refuse("a W value is not finite");
    if (t->n_extern) return refuse("the tape reads user closures (L_EXTERN): evaluate it on the host side and call sdf_contour_grid_host");
    return contour_run(who, t->ctx, t, dim, nullptr, h_values, X, nx, Y, ny, W, nw, level, out, counts);
}

int sdf_contours_fetch(sdf_contours *r, double *h_points, int64_t *h_offsets, uint8_t *h_closed, int32_t *h_layer, double *h_area) {
    if (!r) { fail("sdf_contours_fetch: NULL argument"); return 2; }
    sdf_ctx *c = r->ctx;
    HIPCHK_FN(set_device(c->device));
    if (r->n_contours < 1) {                                           // nothing on the device
        if (h_offsets) h_offsets[0] = 0;
        return 0;
    }
    const char *base = r->block.as<char>();
    const size_t nc = (size_t)r->n_contours;
    if (h_points) HIPCHK_FN(hipMemcpyAsync(h_points, base, (size_t)r->n_points * 16, hipMemcpyDeviceToHost, c->stream));
    if (h_offsets) HIPCHK_FN(hipMemcpyAsync(h_offsets, base + r->o_offsets, (nc + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_closed) HIPCHK_FN(hipMemcpyAsync(h_closed, base + r->o_closed, nc, hipMemcpyDeviceToHost, c->stream));
    if (h_layer) HIPCHK_FN(hipMemcpyAsync(h_layer, base + r->o_layer, nc * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_area) HIPCHK_FN(hipMemcpyAsync(h_area, base + r->o_area, nc * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_FN(stream_wait(c->stream));
    return 0;
}

int sdf_contours_destroy(sdf_contours *r) {
    if (!r) return 0;
    (void)hipSetDevice(r->ctx->device);
    delete r;
    return 0;
}

double sdf_contour_last_kernel_ms(double *parts4) {
    for (int k = 0; parts4 && k < 4; k++) parts4[k] = g_contour_ms[k];
    return g_contour_ms[0] + g_contour_ms[1] + g_contour_ms[2] + g_contour_ms[3];
}

}  // extern "C"
