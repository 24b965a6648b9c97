// sdf_dual.hip -- dual contouring of the field on a dense grid (sdf_generate_dual; added under ABI 17): one
// vertex in every grid cell that the surface crosses, placed by the quadric of the tangent planes at the cell's edge crossings, one
// quad per crossing edge (Ju, Losasso, Schaefer, Warren 2002).  tests/dual_ref.py is the definition and every output is reproduced bit
// for bit: float64, one rounding per written operation (-ffp-contract=off), t = v0 / (v0 - v1), p = lo + t * (hi - lo), the sums of
// a cell sequential over its twelve edges in the definition's order.  The unit holds no tape interpreter: it samples through
// sdf_eval_points and takes the normals at the crossing points through the launcher of k_vertex_normals (sdf_normals.h).
//
// Samples V[nx][ny][nz], s = (i * ny + j) * nz + k, one lane per sample with the lanes along k.  A cell is named by the sample at its
// low corner, so the cells and the samples share one index and one launch shape.
//   k_dual_points      the points of a slab of samples for sdf_eval_points (at most 2^22 per launch)
//   k_dual_classify    per sample: its value and its three +1 neighbours -> the 3-bit crossing flag and its popcount; the edges whose
//                      ends differ in sign but are not both finite are counted (block_add of sdf_block.h, one atomic per workgroup).
//                      A stream with 4 x reuse that the caches serve.  The library scan of the popcounts numbers the crossings by
//                      ascending (s, a): edge index = base[s] + popcount of the lower flags.
//   k_dual_cross       per flagged sample: the crossing points, the (s, a) of every crossing and whether its four cells exist.
//   k_dual_cells       per sample: is one of the twelve edges of its cell a crossing (the flag bytes of seven samples).  The same scan
//                      numbers the active cells.
//   k_dual_cell_list   per sample: an active cell writes its sample index at its number, so that the next kernel runs over the surface
//                      and not over the grid (at 2^27 samples of the example 1.4 million cells are active: one lane per SAMPLE in
//                      k_dual_vertex took 2.56 ms, profiles/dual01_dual_contouring.md).
//   k_dual_vertex      ONE LANE PER ACTIVE CELL gathers its up to twelve crossings in the fixed order (flag and base of four samples
//                      per axis), accumulates the count and the twelve sums in registers, solves (quadric_solve, sdf_dual.h) and
//                      clamps.  Sequential sums, so no float atomic and no dependence on the launch geometry.  The three counters
//                      are flags reduced per workgroup (block_count).  It also marks the block of cells it lies in, for the closing
//                      line's nonempty / empty.
//   k_dual_emit        one lane per crossing writes its two triangles, 18 doubles, at 2 x its rank among the crossings that have four
//                      cells (a second library scan), and their six indices where the caller keeps the parts.
// Device memory: 21 bytes per sample (value 8, counts 4, scan bases of edges and cells 4 + 4, flags 1) and one slab of points; what
// else there is is proportional to the surface: 61 bytes per crossing, 28 per active cell, the soup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "sdf_block.h"
#include "sdf_dual.h"
#include "sdf_internal.h"
#include "sdf_normals.h"
#include "sdf_prims.h"

using namespace sdfk;

namespace {

struct DGrid {
    int n[3];                                                          // (n[0] * n[1] * n[2] < 2^31: every sample index fits an int)
    int stride[3];
};

struct DualHead {
    unsigned long long nonfinite;
    unsigned long long clamped, fallback, flat;                        // (contiguous: one block_count)
};

__device__ __forceinline__ void sample_index(const DGrid &g, int s, int (&i)[3]) {
    i[2] = s % g.n[2];
    const int r = s / g.n[2];
    i[1] = r % g.n[1];
    i[0] = r / g.n[1];
}

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < (double)INFINITY; }       // (false for NaN)

__global__ __launch_bounds__(256) void k_dual_points(const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z,
                                                     const DGrid g, long long s0, int m, double *__restrict__ pts) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= m) return;
    int idx[3];
    sample_index(g, (int)(s0 + i), idx);
    pts[3 * (size_t)i] = X[idx[0]];
    pts[3 * (size_t)i + 1] = Y[idx[1]];
    pts[3 * (size_t)i + 2] = Z[idx[2]];
}

__global__ __launch_bounds__(256) void k_dual_classify(const double *__restrict__ V, const DGrid g, long long n, unsigned char *__restrict__ flags,
                                                       int *__restrict__ cnt, DualHead *head) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned bad[1] = {0u};
    if (s < n) {
        int idx[3];
        sample_index(g, (int)s, idx);
        const double v0 = V[s];
        const bool in0 = v0 < 0.0, fin0 = finite64(v0);
        unsigned f = 0u;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (idx[a] + 1 < g.n[a]) {
                const double v1 = V[s + g.stride[a]];
                const bool differ = in0 != (v1 < 0.0), both = fin0 && finite64(v1);
                if (differ && both) f |= 1u << a;
                if (differ && !both) bad[0] += 1u;
            }
        }
        flags[s] = (unsigned char)f;
        cnt[s] = __popc(f);
    }
    block_add(bad, &head->nonfinite);
}

// per flagged sample: pts n_cross x 3, esample / eaxis the (s, a) of every crossing, qflag whether its four cells exist
__global__ __launch_bounds__(256) void k_dual_cross(const double *__restrict__ V, const double *__restrict__ X, const double *__restrict__ Y,
                                                    const double *__restrict__ Z, const DGrid g, long long n,
                                                    const unsigned char *__restrict__ flags, const int *__restrict__ base, int n_cross,
                                                    double *__restrict__ pts, int *__restrict__ esample, unsigned char *__restrict__ eaxis,
                                                    int *__restrict__ qflag) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const unsigned f = flags[s];
    if (!f) return;
    int idx[3];
    sample_index(g, (int)s, idx);
    const double *ax[3] = {X, Y, Z};
    const double v0 = V[s];
    int e = base[s];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!((f >> a) & 1u)) continue;
        if (e < 0 || e >= n_cross) return;                             // (a base the scan did not write: nothing out of bounds)
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const double v1 = V[s + g.stride[a]];
        const double lo = ax[a][idx[a]], hi = ax[a][idx[a] + 1];
        const double t = v0 / (v0 - v1);
        double p[3] = {X[idx[0]], Y[idx[1]], Z[idx[2]]};
        p[a] = lo + t * (hi - lo);
        pts[3 * (size_t)e] = p[0];
        pts[3 * (size_t)e + 1] = p[1];
        pts[3 * (size_t)e + 2] = p[2];
        esample[e] = (int)s;
        eaxis[e] = (unsigned char)a;
        qflag[e] = (idx[b] >= 1 && idx[c] >= 1 && idx[b] <= g.n[b] - 2 && idx[c] <= g.n[c] - 2) ? 1 : 0;
        e += 1;
    }
}

__global__ __launch_bounds__(256) void k_dual_cells(const unsigned char *__restrict__ flags, const DGrid g, long long n, int *__restrict__ cflag) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    int idx[3];
    sample_index(g, (int)s, idx);
    unsigned any = 0u;
    if (idx[0] + 1 < g.n[0] && idx[1] + 1 < g.n[1] && idx[2] + 1 < g.n[2]) {      // (a cell: its eight corners are samples)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
            for (int k = 0; k < 4; k++) any |= ((unsigned)flags[s + (k & 1) * g.stride[b] + (k >> 1) * g.stride[c]] >> a) & 1u;
        }
    }
    cflag[s] = (int)any;
}

// the active cells as a list: csample[k] = the low-corner sample of active cell k, one lane per sample
__global__ __launch_bounds__(256) void k_dual_cell_list(const int *__restrict__ cflag, const int *__restrict__ cbase, long long n, int n_active,
                                                        int *__restrict__ csample) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n || !cflag[s]) return;
    const int k = cbase[s];
    if (k >= 0 && k < n_active) csample[k] = (int)s;
}

// one lane per active cell (named by its low-corner sample): the sums over its crossings, the solve, the clamp; verts n_active x 3
__global__ __launch_bounds__(256) void k_dual_vertex(const unsigned char *__restrict__ flags, const int *__restrict__ base,
                                                     const int *__restrict__ csample, const double *__restrict__ pts, const double *__restrict__ nrm,
                                                     const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z,
                                                     const DGrid g, long long n, int n_cross, int n_active, double reg, int bs, int nby, int nbz,
                                                     double *__restrict__ verts, unsigned char *__restrict__ block_used, DualHead *head) {
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    bool counts[3] = {false, false, false};                            // clamped, mean_fallback, flat
    const long long s = k < n_active ? (long long)csample[k] : -1;
    int idx[3] = {0, 0, 0};
    if (s >= 0 && s < n) sample_index(g, (int)s, idx);
    if (s >= 0 && s < n && idx[0] + 1 < g.n[0] && idx[1] + 1 < g.n[1] && idx[2] + 1 < g.n[2]) {      // (a cell: what it gathers from are samples)
        const double *ax[3] = {X, Y, Z};
        double ctr[3], half[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double lo = ax[a][idx[a]], hi = ax[a][idx[a] + 1];
            half[a] = 0.5 * (hi - lo);
            ctr[a] = lo + half[a];
        }
        double count = 0.0, sq[3] = {0.0, 0.0, 0.0}, q9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
            for (int j = 0; j < 4; j++) {                              // (db, dc) = (0, 0), (1, 0), (0, 1), (1, 1)
                const long long se = s + (j & 1) * g.stride[b] + (j >> 1) * g.stride[c];
                const unsigned fe = flags[se];
                if (!((fe >> a) & 1u)) continue;
                const int e = base[se] + __popc(fe & ((1u << a) - 1u));
                if (e < 0 || e >= n_cross) continue;
                const double q0 = pts[3 * (size_t)e] - ctr[0], q1 = pts[3 * (size_t)e + 1] - ctr[1], q2 = pts[3 * (size_t)e + 2] - ctr[2];
                const double n0 = nrm[3 * (size_t)e], n1 = nrm[3 * (size_t)e + 1], n2 = nrm[3 * (size_t)e + 2];
                const double d = (n0 * q0 + n1 * q1) + n2 * q2;
                count = count + 1.0;
                sq[0] = sq[0] + q0; sq[1] = sq[1] + q1; sq[2] = sq[2] + q2;
                q9[0] = q9[0] + n0 * n0; q9[1] = q9[1] + n0 * n1; q9[2] = q9[2] + n0 * n2;
                q9[3] = q9[3] + n1 * n1; q9[4] = q9[4] + n1 * n2; q9[5] = q9[5] + n2 * n2;
                q9[6] = q9[6] + n0 * d; q9[7] = q9[7] + n1 * d; q9[8] = q9[8] + n2 * d;
            }
        }
        const double m[3] = {sq[0] / count, sq[1] / count, sq[2] / count};
        double x[3];
        const double w = quadric_solve(q9, m, reg, x);
        const bool is_flat = w == 0.0;
        const bool fell_back = !is_flat && !(finite64(x[0]) && finite64(x[1]) && finite64(x[2]));
        bool clamped = false;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            double xc = x[a] < -half[a] ? -half[a] : x[a];             // np.minimum(np.maximum(x, -h), h) of a finite x
            xc = xc > half[a] ? half[a] : xc;
            clamped = clamped || xc != x[a];
            x[a] = (is_flat || fell_back) ? m[a] : xc;
        }
        counts[0] = clamped && !is_flat && !fell_back; counts[1] = fell_back; counts[2] = is_flat;
        verts[3 * (size_t)k] = ctr[0] + x[0];
        verts[3 * (size_t)k + 1] = ctr[1] + x[1];
        verts[3 * (size_t)k + 2] = ctr[2] + x[2];
        if (bs > 0) block_used[((size_t)(idx[0] / bs) * nby + idx[1] / bs) * nbz + idx[2] / bs] = 1;    // (every lane stores the same byte)
    }
    block_count(counts, &head->clamped);
}

// one lane per crossing: out n_quads x 18 doubles; tri (or NULL) n_quads x 6 vertex indices
__global__ __launch_bounds__(256) void k_dual_emit(const double *__restrict__ V, const int *__restrict__ esample, const unsigned char *__restrict__ eaxis,
                                                   const int *__restrict__ qflag, const int *__restrict__ qpos, const int *__restrict__ cbase,
                                                   const double *__restrict__ verts, const DGrid g, int n_cross, int n_quads, int n_active,
                                                   double *__restrict__ out, long long *__restrict__ tri) {
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= n_cross || !qflag[e]) return;
    const int r = qpos[e];
    if (r < 0 || r >= n_quads) return;
    const int s = esample[e], a = eaxis[e];
    if (a > 2) return;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const int sb = g.stride[b], sc = g.stride[c];
    if (s < sb + sc || (long long)s >= (long long)g.n[0] * g.stride[0]) return;      // (its four cells lie below it: see qflag)
    int q[4] = {cbase[s - sb - sc], cbase[s - sc], cbase[s], cbase[s - sb]};      // (-1, -1), (0, -1), (0, 0), (-1, 0) in (b, c)
    if (!(V[s] < 0.0)) { const int t0 = q[0], t1 = q[1]; q[0] = q[3]; q[1] = q[2]; q[2] = t1; q[3] = t0; }
#pragma unroll
    for (int j = 0; j < 4; j++) if (q[j] < 0 || q[j] >= n_active) return;     // (a cell the scan did not number: nothing out of bounds)
    const int order[6] = {0, 1, 2, 0, 2, 3};
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const int k = q[order[j]];
        out[18 * (size_t)r + 3 * j] = verts[3 * (size_t)k];
        out[18 * (size_t)r + 3 * j + 1] = verts[3 * (size_t)k + 1];
        out[18 * (size_t)r + 3 * j + 2] = verts[3 * (size_t)k + 2];
        if (tri) tri[6 * (size_t)r + j] = k;
    }
}

thread_local double g_dual_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};          // sampling, crossings, normals, cells + vertices, emission

constexpr long long SLAB = 1ll << 22;                                  // the points of one sdf_eval_points launch

}  // namespace

// what a call leaves behind for sdf_dual_parts_fetch: one device block
struct sdf_dual_parts {
    sdf_ctx *ctx = nullptr;
    DevBlock block;                                                    // points, normals, vertices, cells
    long long n_cross = 0, n_active = 0, n_tris = 0;
    size_t o_nrm = 0, o_verts = 0, o_tri = 0;
};

namespace {

struct SoupGuard {                                                     // (a DevBuf has no destructor: a failed call hands the soup back)
    DevBuf soup;
    bool keep = false;
    ~SoupGuard() { if (!keep) soup.release(); }
};

int dual_run(const char *who, sdf_ctx *c, sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, double eps,
             double reg, int bs, sdf_mesh **out, int64_t *counters8, sdf_dual_parts **parts_out) {
    for (int k = 0; k < 8; k++) counters8[k] = 0;
    for (int k = 0; k < 5; k++) g_dual_ms[k] = 0.0;
    sdf_mesh *mesh = new sdf_mesh();
    struct MeshGuard { sdf_mesh *m; ~MeshGuard() { delete m; } } mesh_guard{mesh};
    mesh->ctx = c;
    sdf_dual_parts *parts = new sdf_dual_parts();
    struct PartsGuard { sdf_dual_parts *p; ~PartsGuard() { delete p; } } parts_guard{parts};
    parts->ctx = c;
    SoupGuard sg;
    auto done = [&]() {
        mesh->out = sg.soup;
        sg.keep = true;
        *out = mesh;
        mesh_guard.m = nullptr;
        if (parts_out) { *parts_out = parts; parts_guard.p = nullptr; }
        return 0;
    };
    const long long n = (long long)nx * ny * nz;
    if (nx < 2 || ny < 2 || nz < 2) return done();                     // (no cell: the empty mesh, no launch)
    HIPCHK_MSG(who, set_device(c->device));
    hipStream_t st = c->stream;
    DGrid g;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    g.stride[0] = ny * nz; g.stride[1] = nz; g.stride[2] = 1;
    const int nbx = bs > 0 ? (nx - 1 + bs - 1) / bs : 0, nby = bs > 0 ? (ny - 1 + bs - 1) / bs : 0, nbz = bs > 0 ? (nz - 1 + bs - 1) / bs : 0;
    const long long n_blocks = (long long)nbx * nby * nbz;
    const long long slab = n < SLAB ? n : SLAB;
    const long long max_cross = 3 * n < (1ll << 31) - 1 ? 3 * n : (1ll << 31) - 1;

    // ---- stage 1: what is sized by the grid ----
    DualHead h_head = {};
    std::vector<unsigned char> h_used((size_t)n_blocks);
    size_t tmp_bytes = 0;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n, &tmp_bytes));                // (the crossings are scanned in the second stage's own block)
    double *V, *dX, *dY, *dZ, *spts;
    int *cnt, *base, *cbase;
    unsigned char *flags, *used, *tmp;
    DualHead *head;
    Scratch grid_scratch(st);                                          // (declared after the host copies: it waits for the stream before they go)
    grid_scratch.part(&head, 1);
    grid_scratch.part(&V, (size_t)n);
    grid_scratch.part(&dX, (size_t)nx); grid_scratch.part(&dY, (size_t)ny); grid_scratch.part(&dZ, (size_t)nz);
    grid_scratch.part(&spts, (size_t)slab * 3);
    grid_scratch.part(&cnt, (size_t)n); grid_scratch.part(&base, (size_t)n); grid_scratch.part(&cbase, (size_t)n);
    grid_scratch.part(&flags, (size_t)n);
    grid_scratch.part(&used, (size_t)(n_blocks > 0 ? n_blocks : 1));
    grid_scratch.part(&tmp, tmp_bytes);
    size_t free_b = 0;
    bool fits = false;
    HIPCHK_MSG(who, mem_fits(grid_scratch.bytes, &fits, &free_b));
    if (!fits)
        return fail(std::string(who) + "the grid of " + std::to_string(n) + " samples needs " + std::to_string(grid_scratch.bytes) +
                    " bytes of device memory, " + std::to_string(free_b) + " are free");
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(grid_scratch.bytes) + "): ", grid_scratch.alloc());
    HIPCHK_MSG(who, hipMemcpyAsync(dX, X, (size_t)nx * 8, hipMemcpyHostToDevice, st));
    HIPCHK_MSG(who, hipMemcpyAsync(dY, Y, (size_t)ny * 8, hipMemcpyHostToDevice, st));
    HIPCHK_MSG(who, hipMemcpyAsync(dZ, Z, (size_t)nz * 8, hipMemcpyHostToDevice, st));
    HIPCHK_MSG(who, hipMemsetAsync(head, 0, sizeof(DualHead), st));
    HIPCHK_MSG(who, hipMemsetAsync(used, 0, (size_t)(n_blocks > 0 ? n_blocks : 1), st));
    EventTimer t_sample, t_cross, t_normals, t_vertex, t_emit;
    HIPCHK_MSG(who, t_sample.start(st));
    for (long long s0 = 0; s0 < n; s0 += slab) {
        const long long m = n - s0 < slab ? n - s0 : slab;
        HIPCHK_MSG(who, launch_rows(k_dual_points, m, st, dX, dY, dZ, g, s0, (int)m, spts));
        if (sdf_eval_points(t, spts, m, 3, V + s0, SDF_PRECISION_F64)) return 1;
    }
    HIPCHK_MSG(who, t_sample.stop(st));

    // ---- the crossing edges: flags, counts, numbers ----
    HIPCHK_MSG(who, t_cross.start(st));
    HIPCHK_MSG(who, launch_rows(k_dual_classify, n, st, V, g, n, flags, cnt, head));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(DualHead), hipMemcpyDeviceToHost, st));          // (lands behind the scan's wait)
    long long n_cross = 0;
    if (number_counts(who, "crossing counts", st, cnt, base, n, max_cross, tmp, tmp_bytes, &n_cross)) return 1;
    counters8[4] = (int64_t)h_head.nonfinite;
    if (n_cross == 0) {
        HIPCHK_MSG(who, t_cross.stop(st));
        HIPCHK_MSG(who, stream_wait(st));
        HIPCHK_MSG(who, t_sample.ms(&g_dual_ms[0]));
        HIPCHK_MSG(who, t_cross.ms(&g_dual_ms[1]));
        mesh->st.n_batches = n_blocks; mesh->st.n_empty = n_blocks;
        return done();
    }

    // ---- stage 2: what is sized by the crossings ----
    size_t tmp2_bytes = 0;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n_cross, &tmp2_bytes));
    int *esample, *qflag, *qpos;
    unsigned char *eaxis, *tmp2;
    unsigned long long *d_flat;
    Scratch cross_scratch(st);
    cross_scratch.part(&esample, (size_t)n_cross); cross_scratch.part(&qflag, (size_t)n_cross); cross_scratch.part(&qpos, (size_t)n_cross);
    cross_scratch.part(&eaxis, (size_t)n_cross);
    cross_scratch.part(&d_flat, 1);
    cross_scratch.part(&tmp2, tmp2_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(cross_scratch.bytes) + "): ", cross_scratch.alloc());
    DevBlock pn;                                                       // the crossing points and normals
    const size_t pn_half = align256((size_t)n_cross * 24);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(2 * pn_half) + "): ", pn.alloc(2 * pn_half, st));
    double *pts = pn.as<double>(), *nrm = (double *)(pn.as<char>() + pn_half);
    HIPCHK_MSG(who, launch_rows(k_dual_cross, n, st, V, dX, dY, dZ, g, n, flags, base, (int)n_cross, pts, esample, eaxis, qflag));
    long long n_quads = 0;
    if (number_flags(who, "quad flags", st, qflag, qpos, n_cross, tmp2, tmp2_bytes, &n_quads)) return 1;
    HIPCHK_MSG(who, t_cross.stop(st));
    HIPCHK_MSG(who, t_normals.start(st));
    HIPCHK_MSG(who, hipMemsetAsync(d_flat, 0, 8, st));
    HIPCHK_MSG(who, (hipError_t)launch_vertex_normals(st, t->d_code, t->d_c64, t->full, pts, n_cross, eps, nrm, d_flat));
    HIPCHK_MSG(who, t_normals.stop(st));

    // ---- the active cells and their vertices ----
    HIPCHK_MSG(who, t_vertex.start(st));
    int *cflag = cnt;                                                  // (the counts have been scanned: the part serves the cells' flags)
    HIPCHK_MSG(who, launch_rows(k_dual_cells, n, st, flags, g, n, cflag));
    long long n_active = 0;
    if (number_flags(who, "cell flags", st, cflag, cbase, n, tmp, tmp_bytes, &n_active)) return 1;
    if (n_active < 1) return fail(std::string(who) + "crossings without an active cell");
    const long long n_tris = 2 * n_quads;
    const bool keep = parts_out != nullptr;
    DevBlock vt;                                                       // the vertices and, for a caller that keeps the parts, the cells
    const size_t v_bytes = align256((size_t)n_active * 24);
    const size_t vt_bytes = v_bytes + (keep ? align256((size_t)(n_tris > 0 ? n_tris : 1) * 24) : 0);     // (what a caller that keeps the parts is handed)
    const size_t list_bytes = align256((size_t)n_active * 4);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(vt_bytes + list_bytes) + "): ", vt.alloc(vt_bytes + list_bytes, st));
    double *verts = vt.as<double>();
    long long *tri = keep ? (long long *)(vt.as<char>() + v_bytes) : nullptr;
    int *csample = (int *)(vt.as<char>() + vt_bytes);
    HIPCHK_MSG(who, launch_rows(k_dual_cell_list, n, st, cflag, cbase, n, (int)n_active, csample));
    HIPCHK_MSG(who, launch_rows(k_dual_vertex, n_active, st, flags, base, csample, pts, nrm, dX, dY, dZ, g, n, (int)n_cross, (int)n_active, reg, bs,
                                nby, nbz, verts, used, head));
    HIPCHK_MSG(who, t_vertex.stop(st));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(DualHead), hipMemcpyDeviceToHost, st));
    if (n_blocks > 0) HIPCHK_MSG(who, hipMemcpyAsync(h_used.data(), used, (size_t)n_blocks, hipMemcpyDeviceToHost, st));

    // ---- two triangles per crossing that has its four cells ----
    HIPCHK_MSG(who, t_emit.start(st));
    if (n_quads > 0) {
        if (sg.soup.ensure((size_t)n_tris * 72)) return 1;
        HIPCHK_MSG(who, launch_rows(k_dual_emit, n_cross, st, V, esample, eaxis, qflag, qpos, cbase, verts, g, (int)n_cross, (int)n_quads,
                                    (int)n_active, (double *)sg.soup.p, tri));
    }
    HIPCHK_MSG(who, t_emit.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, t_sample.ms(&g_dual_ms[0]));
    HIPCHK_MSG(who, t_cross.ms(&g_dual_ms[1]));
    HIPCHK_MSG(who, t_normals.ms(&g_dual_ms[2]));
    HIPCHK_MSG(who, t_vertex.ms(&g_dual_ms[3]));
    HIPCHK_MSG(who, t_emit.ms(&g_dual_ms[4]));
    counters8[0] = (int64_t)n_cross;
    counters8[1] = (int64_t)n_active;
    counters8[2] = (int64_t)n_tris;
    counters8[3] = (int64_t)(n_cross - n_quads);
    counters8[5] = (int64_t)h_head.clamped;
    counters8[6] = (int64_t)h_head.fallback;
    counters8[7] = (int64_t)h_head.flat;
    long long nonempty = 0;
    for (unsigned char u : h_used) nonempty += u ? 1 : 0;
    mesh->st.n_batches = n_blocks; mesh->st.n_nonempty = nonempty; mesh->st.n_empty = n_blocks - nonempty;
    mesh->st.n_triangles = n_tris;
    mesh->st.n_grid_voxels = (long long)(nx - 1) * (ny - 1) * (nz - 1);
    mesh->st.n_eval_voxels = mesh->st.n_grid_voxels;
    mesh->st.n_sampled_voxels = n;
    mesh->st.ms_total = g_dual_ms[0] + g_dual_ms[1] + g_dual_ms[2] + g_dual_ms[3] + g_dual_ms[4];
    if (keep) {                                                        // one block for the fetch: points, normals, vertices, cells
        parts->n_cross = n_cross; parts->n_active = n_active; parts->n_tris = n_tris;
        parts->o_nrm = pn_half; parts->o_verts = 2 * pn_half; parts->o_tri = 2 * pn_half + v_bytes;
        const size_t bytes = 2 * pn_half + vt_bytes;
        HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(bytes) + "): ", parts->block.alloc(bytes, st));
        HIPCHK_MSG(who, hipMemcpyAsync(parts->block.as<char>(), pn.as<char>(), 2 * pn_half, hipMemcpyDeviceToDevice, st));
        HIPCHK_MSG(who, hipMemcpyAsync(parts->block.as<char>() + 2 * pn_half, vt.as<char>(), vt_bytes, hipMemcpyDeviceToDevice, st));
        HIPCHK_MSG(who, stream_wait(st));
    }
    return done();
}

}  // namespace

extern "C" {

int sdf_generate_dual(sdf_ctx *c, sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, double eps, double reg,
                      int block, sdf_mesh **out, int64_t *h_counters8, sdf_dual_parts **parts) {
    static const char who[] = "sdf_generate_dual: ";
    auto refuse = [&](const std::string &why) { fail(std::string(who) + why); return 2; };
    if (!c || !t || !X || !Y || !Z || !out || !h_counters8) return refuse("NULL argument");
    *out = nullptr;
    if (parts) *parts = nullptr;
    if (t->ctx != c) return refuse("the tape belongs to another context");
    if (nx < 0 || ny < 0 || nz < 0) return refuse("a negative axis length");
    if ((double)nx * (double)ny * (double)nz >= 2147483648.0) return refuse("2^31 or more samples");
    if (!(std::isfinite(eps) && eps > 0.0)) return refuse("eps must be finite and positive");
    if (!(std::isfinite(reg) && reg >= 0.0)) return refuse("reg must be finite and not negative");
    for (int k = 0; k < nx; k++) if (!std::isfinite(X[k])) return refuse("an X value is not finite");
    for (int k = 0; k < ny; k++) if (!std::isfinite(Y[k])) return refuse("a Y value is not finite");
    for (int k = 0; k < nz; k++) if (!std::isfinite(Z[k])) return refuse("a Z value is not finite");
    if (t->n_extern) return refuse("the tape reads user closures (L_EXTERN): take the normals over sdf_eval_points_extern_host");
    return dual_run(who, c, t, X, nx, Y, ny, Z, nz, eps, reg, block, out, h_counters8, parts);
}

int sdf_dual_parts_fetch(sdf_dual_parts *p, double *h_points, double *h_normals, double *h_vertices, int64_t *h_cells) {
    if (!p) { fail("sdf_dual_parts_fetch: NULL argument"); return 2; }
    if (p->n_cross < 1) return 0;                                      // nothing on the device
    sdf_ctx *c = p->ctx;
    HIPCHK_FN(set_device(c->device));
    const char *base = p->block.as<char>();
    if (h_points) HIPCHK_FN(hipMemcpyAsync(h_points, base, (size_t)p->n_cross * 24, hipMemcpyDeviceToHost, c->stream));
    if (h_normals) HIPCHK_FN(hipMemcpyAsync(h_normals, base + p->o_nrm, (size_t)p->n_cross * 24, hipMemcpyDeviceToHost, c->stream));
    if (h_vertices) HIPCHK_FN(hipMemcpyAsync(h_vertices, base + p->o_verts, (size_t)p->n_active * 24, hipMemcpyDeviceToHost, c->stream));
    if (h_cells && p->n_tris > 0) HIPCHK_FN(hipMemcpyAsync(h_cells, base + p->o_tri, (size_t)p->n_tris * 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_FN(stream_wait(c->stream));
    return 0;
}

int sdf_dual_parts_destroy(sdf_dual_parts *p) {
    if (!p) return 0;
    (void)hipSetDevice(p->ctx->device);
    delete p;
    return 0;
}

double sdf_generate_dual_last_kernel_ms(double *parts5) {
    for (int k = 0; parts5 && k < 5; k++) parts5[k] = g_dual_ms[k];
    return g_dual_ms[0] + g_dual_ms[1] + g_dual_ms[2] + g_dual_ms[3] + g_dual_ms[4];
}

}  // extern "C"
