// sdf_mesh_out.hip -- what reads a finished mesh and needs no tape: collecting a call in flight, statistics, the soup on the device and
// on the host (float64, 16-byte records expanded by host threads, STL records), batch offsets, the weld, binary PLY records, the moments
// and the edge census, the connected shells and a selection of them, the simplified mesh, the mended mesh, the rating of build
// directions, kinds, prune masks, and the end of a mesh.  (The entries that take a tape to the mesh live in sdf_probe_out.hip.)
// Launches only through the launchers of sdf_plain.h, sdf_measure.h, sdf_components.h, sdf_simplify.h, sdf_mend.h, sdf_overhang.h and
// sdf_weld.hip: built WITHOUT the interpreters' structurizer option (build.units).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sdf_internal.h"
#include "sdf_components.h"
#include "sdf_expand_host.h"   // (+ <chrono>, <cstring>, <mutex>, <thread>)
#include "sdf_measure.h"
#include "sdf_mend.h"
#include "sdf_overhang.h"
#include "sdf_plain.h"
#include "sdf_simplify.h"

using namespace sdfk;

// (sdf_internal.h) the float64 soup of a records mesh, made on the device by k_expand, once
int ensure_soup(sdf_mesh *m) {
    if (!m->records || m->out.p || m->st.n_triangles == 0) return 0;
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    if (m->out.ensure((size_t)m->st.n_triangles * 72)) return 1;
    SlabPtrs ptrs = {};
    ptrs.p[0] = (const unsigned char *)m->slab.p;
    HIPCHK((hipError_t)sdf_launch_expand(c->stream, ptrs, 1, m->slab_items, m->slab_tris, (double *)m->out.p, (unsigned long long)m->st.n_triangles));
    return 0;
}

// (Cutting a large device-to-host copy into pieces that travel on several streams at once was measured in r02: the
// 212 MB soup took 7.7 ms as one copy, 8.7 ms as two, 9.8 ms as four -- one copy already runs at the link's rate for
// pinned memory (28 GB/s on the test boxes).  A kernel that stores straight into the mapped pinned block, 32 to 2048
// workgroups: the same 7.5 ms.  One copy it stays.)
int copy_to_host(sdf_ctx *c, void *h_dst, const void *d_src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    return 0;
}

// (sdf_internal.h) the refusals of a list of build directions: the overhang entries below, sdf_mesh_support_rays
int overhang_refused(const char *who, const double *h_dirs, long long n_dirs, double sin_limit, double bed_tol) {
    const std::string w(who);
    if (n_dirs < 1) return fail(w + ": n_dirs must be at least 1");
    if (n_dirs > OVERHANG_MAX_DIRS) return fail(w + ": more than 2^20 directions");
    if (!(sin_limit >= 0.0 && sin_limit < 1.0)) return fail(w + ": sin_limit must lie in [0, 1)");
    if (!(bed_tol >= 0.0)) return fail(w + ": bed_tol must not be negative or NaN");
    for (long long k = 0; k < n_dirs; k++) {
        const double x = h_dirs[3 * k], y = h_dirs[3 * k + 1], z = h_dirs[3 * k + 2];
        const double len = std::sqrt((x * x + y * y) + z * z);
        if (!(std::fabs(len - 1.0) <= 1e-12))                          // (a NaN or an infinite component fails this too)
            return fail(w + ": direction " + std::to_string(k) + " is zero, not finite or not of unit length to 1e-12");
    }
    return 0;
}

extern "C" {

int sdf_mesh_wait(sdf_mesh *m, int *emitted) {
    if (!m) return fail("sdf_mesh_wait: NULL argument");
    sdf_mesh::Pending &pd = m->pend;
    if (pd.active) {
        sdf_ctx *c = m->ctx;
        HIPCHK(set_device(c->device));
        CallSlot &cs = c->slots[pd.got.slot];
        HIPCHK(event_wait(cs.done));
        pd.active = false;
        const bool slab = pd.call.dest == GenCall::SLAB;
        MeshCounters h;
        const int rc = finish_call(m, pd.call, pd.got, slab, h);
        cs.busy = false; cs.owner = nullptr;      // (everything the slot held for this mesh has been read)
        if (rc) return 1;
        if (h.overflow && slab) {
            // a slab that was too small: the exchange protocol retries with larger slabs on EVERY rank (sdf_amd/dist.py)
            m->emitted_to = nullptr;
        } else if (h.overflow) {
            // the soup did not fit the caller's buffer: the call is repeated synchronously into library memory
            // (sized from the count just learned)
            pd.call.tape->hint_key = pd.got.key; pd.call.tape->hint_total_tris = std::max<unsigned long long>(h.total, 1);
            GenCall again = pd.call;
            again.dest = GenCall::SOUP; again.d_out = nullptr; again.cap_tris = 0;
            again.collected = false;
            if (generate_impl(m, again)) return 1;
            m->st.n_retries += 1;
        } else {
            m->emitted_to = slab ? nullptr : pd.call.d_out;
            m->st.n_retries = 0;
        }
        pd.axes.clear(); pd.axes.shrink_to_fit();
    }
    if (emitted) *emitted = (m->emitted_to != nullptr || m->st.n_triangles == 0) ? 1 : 0;
    return 0;
}

int sdf_mesh_stats(sdf_mesh *m, sdf_stats *out) {
    if (!m || !out) return fail("sdf_mesh_stats: NULL argument");
    MESH_READY(m);
    *out = m->st;
    return 0;
}

int64_t sdf_mesh_triangles(sdf_mesh *m) {
    if (!m) return 0;
    if (m->pend.active && sdf_mesh_wait(m, nullptr)) return -1;
    return m->st.n_triangles;
}

int sdf_mesh_emit_device(sdf_mesh *m, void *d_out) {
    if (!m || !d_out) return fail("sdf_mesh_emit_device: NULL argument");
    MESH_READY(m);
    MESH_SOUP_READY(m);
    sdf_ctx *c = m->ctx;
    if (m->st.n_triangles == 0 || d_out == mesh_soup(m)) return 0;
    HIPCHK(set_device(c->device));
    HIPCHK(hipEventRecord(c->ev[3], c->stream));
    HIPCHK(hipMemcpyAsync(d_out, mesh_soup(m), (size_t)m->st.n_triangles * 72, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev[4], c->stream));
    HIPCHK(stream_wait(c->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[3], c->ev[4]));
    m->st.ms_emit = ms;
    return 0;
}

// The soup on the host.  A mesh of sdf_generate_records sends its RECORDS (16 bytes per triangle + a transform per work item) and the
// float64 soup is made where it is wanted, by `workers` host threads (<= 0: as many as the machine has, at most 32 -- a caller's number: at most 64; the reference's
// `workers=` argument, sdf/core.py:87) -- block by block while the later records are still on the link: the pieces of the copy are
// followed by events, the calling thread publishes how far the records have arrived and takes blocks itself in between.  The
// arithmetic is k_expand's (`double(local) * scale + offset` on the same operands): the soup is the one the device would write.
// Any other mesh: one copy of the float64 soup, as before (`workers` is ignored).
int sdf_mesh_emit_host_workers(sdf_mesh *m, double *h_out, int workers) {
    if (!m || !h_out) return fail("sdf_mesh_emit_host: NULL argument");
    MESH_READY(m);
    if (m->st.n_triangles == 0) return 0;
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    if (!m->records || m->out.p) return copy_to_host(c, h_out, mesh_soup(m), (size_t)m->st.n_triangles * 72);
    const long long nt = m->st.n_triangles, ni = (long long)m->work_end - m->work_begin, nraw = std::min<long long>(m->n_raw, SlabLayout(m->slab_items, m->slab_tris).raw_cap);
    const SlabLayout L(m->slab_items, m->slab_tris);
    // pinned staging: [prefix ni x 8 | transforms ni x 48 | raw area nraw x 36 | records nt x 16]
    const size_t off_xf = (size_t)ni * 8, off_raw = off_xf + (size_t)ni * 48, off_rec = (off_raw + (size_t)nraw * 36 + 63) & ~(size_t)63;
    const size_t need = off_rec + (size_t)nt * 16;
    if (c->h_rec_bytes < need) {
        if (c->h_rec) (void)hipHostFree(c->h_rec);
        c->h_rec = nullptr; c->h_rec_bytes = 0;
        const size_t want = need + need / 8 + (1u << 20);
        if (host_malloc(&c->h_rec, want) != hipSuccess) { c->h_rec = nullptr; return fail("sdf_mesh_emit_host: pinned staging for the records"); }
        c->h_rec_bytes = want;
    }
    char *hs = (char *)c->h_rec;
    const char *slab = (const char *)m->slab.p;
    // the pieces: head (prefix, transforms, raw area) first, then the records in ~ 12 pieces of whole blocks
    sdfhost::ExpandJob job;
    static const long long rec_block = [] { const char *e = getenv("SDF_REC_BLOCK"); return e && atoll(e) >= 64 ? atoll(e) : 8192ll; }();     // (tuning)
    static const long long rec_pieces = [] { const char *e = getenv("SDF_REC_PIECES"); return e && atoll(e) >= 1 ? std::min(atoll(e), 64ll) : 12ll; }();
    job.block = rec_block;
    const long long nblk = (nt + job.block - 1) / job.block;
    const long long blk_per_piece = std::max<long long>(8, (nblk + rec_pieces - 1) / rec_pieces);
    const int npieces = (int)((nblk + blk_per_piece - 1) / blk_per_piece);
    while ((int)c->rec_ev.size() < npieces + 1) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->rec_ev.push_back(e);
    }
    hipStream_t st = c->stream;
    static const bool rec_trace = getenv("SDF_REC_TRACE") != nullptr;   // (diagnostics: when the pieces arrived, when the last block was written)
    const auto tr0 = std::chrono::steady_clock::now();
    auto tr_us = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr0).count(); };
    // (r06j - r06l, 2 x 64 cores: 8 threads are bound by their own arithmetic (47 us per block of 8192 triangles, 2.2 ms), 32 by the memory
    // the block lies in (138 us per block, 1.8 ms), 64 are no faster and have outliers: the machine's count is capped at 32, a caller's at 64)
    int nthreads = workers > 0 ? std::min(workers, 64) : std::min((int)std::thread::hardware_concurrency(), 32);
    nthreads = std::max(1, nthreads);
    nthreads = (int)std::min<long long>(nthreads, std::max<long long>(nblk, 1));
    job.prefix = (const unsigned long long *)hs; job.xf = (const double *)(hs + off_xf);
    job.raw = (const float *)(hs + off_raw); job.raw_cap = std::max<long long>(nraw, 1);
    job.recs = (const Tri16 *)(hs + off_rec);
    job.n_items = ni; job.n_tris = nt; job.out = h_out;
    std::vector<float> blk_trace;
    if (rec_trace) { blk_trace.assign((size_t)2 * nblk, 0.0f); job.trace = blk_trace.data(); job.t_origin = tr0; }
    static std::mutex expand_mu;                         // (ONE expansion at a time per process: the pool serves one job)
    std::lock_guard<std::mutex> expand_lock(expand_mu);
    sdfhost::Pool &pool = sdfhost::Pool::get();
    pool.start(job, nthreads - 1);                       // (the helpers wake up while the copies are enqueued; this thread is one of the workers too)
    // (from here on the helpers hold the job: an error while the copies are enqueued lets them go before it returns)
    struct Helpers { sdfhost::Pool &pool; sdfhost::ExpandJob &job; bool held; ~Helpers() { if (held) { job.abort.store(1); pool.wait(job); } } } helpers{pool, job, true};
    HIPCHK(hipMemcpyAsync(hs, slab + L.prefix_off, (size_t)ni * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + off_xf, slab + L.xf_off, (size_t)ni * 48, hipMemcpyDeviceToHost, st));
    if (nraw) HIPCHK(hipMemcpyAsync(hs + off_raw, slab + L.raw_off, (size_t)nraw * 36, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->rec_ev[0], st));
    for (int k = 0; k < npieces; k++) {
        const long long t0 = (long long)k * blk_per_piece * job.block, t1 = std::min(nt, t0 + blk_per_piece * job.block);
        HIPCHK(hipMemcpyAsync(hs + off_rec + (size_t)t0 * 16, slab + L.tris_off + (size_t)t0 * 16, (size_t)(t1 - t0) * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(c->rec_ev[(size_t)k + 1], st));
    }
    helpers.held = false;
    const double t_enq = tr_us();
    double t_piece[16] = {};
    hipError_t err = event_wait(c->rec_ev[0]);
    const double t_head = tr_us();
    for (int k = 0; k < npieces && err == hipSuccess; k++) {
        err = event_wait(c->rec_ev[(size_t)k + 1]);
        if (err == hipSuccess) job.avail.store(std::min(nt, (long long)(k + 1) * blk_per_piece * job.block), std::memory_order_release);
        if (k < 16) t_piece[k] = tr_us();
    }
    if (err != hipSuccess) job.abort.store(1);
    else sdfhost::expand_work(job);
    const double t_own = tr_us();
    pool.wait(job);
    if (rec_trace) {
        fprintf(stderr, "[records] %lld triangles, %d threads, %d pieces: enqueued %.0f us, head %.0f, pieces", nt, nthreads, npieces, t_enq, t_head);
        for (int k = 0; k < npieces && k < 16; k++) fprintf(stderr, " %.0f", t_piece[k]);
        fprintf(stderr, "; own share done %.0f, all done %.0f us\n", t_own, tr_us());
        double dur = 0, dmax = 0;
        for (long long b = 0; b < nblk; b++) { const double d = blk_trace[2 * b + 1] - blk_trace[2 * b]; dur += d; dmax = std::max(dmax, d); }
        fprintf(stderr, "[records] %lld blocks of %lld triangles: %.0f us each on average (max %.0f); block: started / written, every %lld-th:", nblk, job.block, dur / std::max<long long>(nblk, 1), dmax, std::max<long long>(nblk / 24, 1));
        for (long long b = 0; b < nblk; b += std::max<long long>(nblk / 24, 1)) fprintf(stderr, " %lld: %.0f / %.0f", b, blk_trace[2 * b], blk_trace[2 * b + 1]);
        fprintf(stderr, "\n");
    }
    if (err != hipSuccess) return fail(std::string("sdf_mesh_emit_host: copying the records: ") + hipGetErrorString(err));
    return 0;
}

int sdf_mesh_emit_host(sdf_mesh *m, double *h_out) { return sdf_mesh_emit_host_workers(m, h_out, 0); }

int sdf_mesh_emit_host_range(sdf_mesh *m, int64_t first_tri, int64_t n_tris, double *h_out) {
    if (!m || !h_out) return fail("sdf_mesh_emit_host_range: NULL argument");
    MESH_READY(m);
    if (first_tri < 0 || n_tris < 0 || first_tri + n_tris > m->st.n_triangles) return fail("sdf_mesh_emit_host_range: range outside the soup");
    if (n_tris == 0) return 0;
    MESH_SOUP_READY(m);
    HIPCHK(set_device(m->ctx->device));
    HIPCHK(hipMemcpyAsync(h_out, (const char *)mesh_soup(m) + (size_t)first_tri * 72, (size_t)n_tris * 72, hipMemcpyDeviceToHost, m->ctx->stream));
    HIPCHK(stream_wait(m->ctx->stream));
    return 0;
}

// Where each batch's triangles sit in this shard's soup: after k_mesh every work item's look-back word holds
// the inclusive prefix of the triangle counts up to and including it (ordered_base / publish_count).
int sdf_mesh_batch_offsets(sdf_mesh *m, int64_t *h_out) {
    if (!m || !h_out) return fail("sdf_mesh_batch_offsets: NULL argument");
    MESH_READY(m);
    const int64_t nb = m->st.n_batches;
    for (int64_t b = 0; b <= nb; b++) h_out[b] = 0;
    const int nw = m->work_end - m->work_begin;
    if (nb == 0 || nw <= 0) return 0;
    if (!m->status.p || !m->worklist.p) return fail("sdf_mesh_batch_offsets: this mesh was not produced by sdf_generate");
    HIPCHK(set_device(m->ctx->device));
    std::vector<int> wl((size_t)nw);
    std::vector<unsigned long long> stw((size_t)nw);
    HIPCHK(hipMemcpyAsync(wl.data(), (const int *)m->worklist.p + m->work_begin, (size_t)nw * 4, hipMemcpyDeviceToHost, m->ctx->stream));
    HIPCHK(hipMemcpyAsync(stw.data(), (const unsigned long long *)m->status.p + m->work_begin, (size_t)nw * 8, hipMemcpyDeviceToHost, m->ctx->stream));
    HIPCHK(stream_wait(m->ctx->stream));
    // h_out[b + 1] = triangles of batch b for now; the running sum follows
    unsigned long long prev = 0;
    for (int i = 0; i < nw; i++) {
        if ((stw[(size_t)i] >> 62) != 2ull) return fail("sdf_mesh_batch_offsets: a work item has no prefix (the meshing pass did not complete)");
        const unsigned long long incl = stw[(size_t)i] & MESH_VAL_MASK;
        if (incl < prev || wl[(size_t)i] < 0 || wl[(size_t)i] >= nb) return fail("sdf_mesh_batch_offsets: inconsistent look-back words");
        h_out[wl[(size_t)i] + 1] = (int64_t)(incl - prev);
        prev = incl;
    }
    for (int64_t b = 0; b < nb; b++) h_out[b + 1] += h_out[b];
    return 0;
}

int sdf_mesh_adopt_soup(sdf_ctx *c, const void *d_soup, int64_t n_tris, sdf_mesh **out) {
    if (!c || !out || n_tris < 0 || (n_tris > 0 && !d_soup)) return fail("sdf_mesh_adopt_soup: NULL argument or negative count");
    *out = nullptr;
    sdf_mesh *m = new sdf_mesh();
    m->ctx = c;
    m->emitted_to = const_cast<void *>(d_soup);
    m->st.n_triangles = n_tris;
    *out = m;
    return 0;
}

int sdf_mesh_emit_stl_host(sdf_mesh *m, void *h_out) {
    if (!m || !h_out) return fail("sdf_mesh_emit_stl_host: NULL argument");
    MESH_READY(m);
    const long long nt = m->st.n_triangles;
    if (nt == 0) return 0;
    MESH_SOUP_READY(m);
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    if (c->scratch_out.ensure((size_t)nt * 50)) return 1;
    launch_k_stl(dim3((unsigned)((nt + 255) / 256)), dim3(256), c->stream, (const double *)mesh_soup(m), nt,
                       (unsigned short *)c->scratch_out.p);
    HIPCHK(hipGetLastError());
    return copy_to_host(c, h_out, c->scratch_out.p, (size_t)nt * 50);
}

int sdf_mesh_weld(sdf_mesh *m, int64_t *n_unique) {
    if (!m || !n_unique) return fail("sdf_mesh_weld: NULL argument");
    MESH_READY(m);
    MESH_SOUP_READY(m);
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    if (m->weld_n < 0) {
        long long nu = 0;
        if (weld_device(c->stream, (const double *)mesh_soup(m), 3ll * (long long)m->st.n_triangles, &m->weld_pts, &m->weld_inv, &nu)) return 1;
        m->weld_n = nu;
    }
    *n_unique = (int64_t)m->weld_n;
    return 0;
}

int sdf_mesh_weld_fetch(sdf_mesh *m, double *h_points, int64_t *h_cells) {
    if (!m || !h_points || !h_cells) return fail("sdf_mesh_weld_fetch: NULL argument");
    if (m->weld_n < 0) return fail("sdf_mesh_weld_fetch: call sdf_mesh_weld first");
    if (m->weld_n == 0) return 0;
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    HIPCHK(hipMemcpyAsync(h_points, m->weld_pts.as<double>(), (size_t)m->weld_n * 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_cells, m->weld_inv.as<long long>(), (size_t)m->st.n_triangles * 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    return 0;
}

// ---- the mesh measured on the device: moments of the soup, edge census of the welded cells ----
static thread_local double g_measure_kernel_ms = 0.0;

int sdf_mesh_moments(sdf_mesh *m, const double *origin, sdf_moments *out) {
    if (!m || !out) { fail("sdf_mesh_moments: NULL argument"); return 2; }
    MESH_READY(m);
    *out = sdf_moments();
    for (int k = 0; k < 3; k++) { out->origin[k] = origin ? origin[k] : 0.0; out->box_lo[k] = INFINITY; out->box_hi[k] = -INFINITY; }
    if (m->st.n_triangles == 0) return 0;
    MESH_SOUP_READY(m);
    HIPCHK(set_device(m->ctx->device));
    return measure_moments(m->ctx->stream, (const double *)mesh_soup(m), (long long)m->st.n_triangles, origin, out, &g_measure_kernel_ms);
}

int sdf_mesh_edge_census(sdf_mesh *m, sdf_edge_census *out) {
    if (!m || !out) { fail("sdf_mesh_edge_census: NULL argument"); return 2; }
    if (m->weld_n < 0) { fail("sdf_mesh_edge_census: call sdf_mesh_weld first"); return 2; }
    const long long nt = (long long)m->st.n_triangles;
    if (3 * nt >= (1ll << 31) || m->weld_n >= (1ll << 31)) { fail("sdf_mesh_edge_census: 2^31 or more half-edges or vertices"); return 2; }
    *out = sdf_edge_census();
    out->vertices = (int64_t)m->weld_n;
    out->euler = out->vertices;
    out->closed = out->oriented = 1;
    if (nt == 0) return 0;
    HIPCHK(set_device(m->ctx->device));
    return measure_edge_census(m->ctx->stream, m->weld_inv.as<long long>(), nt, m->weld_n, out, &g_measure_kernel_ms);
}

double sdf_mesh_measure_last_kernel_ms(void) { return g_measure_kernel_ms; }

// ---- the connected shells of the welded mesh, and a selection of them as a mesh of its own ----
static thread_local double g_components_kernel_ms = 0.0;

int sdf_mesh_components(sdf_mesh *m, sdf_components *out) {
    if (!m || !out) { fail("sdf_mesh_components: NULL argument"); return 2; }
    MESH_READY(m);
    *out = sdf_components();
    int64_t nu = 0;
    if (sdf_mesh_weld(m, &nu)) return 1;
    const long long nt = (long long)m->st.n_triangles;
    if (nt >= (1ll << 31) || m->weld_n >= (1ll << 31)) { fail("sdf_mesh_components: 2^31 or more triangles or vertices"); return 2; }
    out->n_vertices = (int64_t)m->weld_n;
    out->n_triangles = (int64_t)nt;
    if (nt == 0) { m->n_shells = 0; return 0; }
    if (m->n_shells < 0) {
        HIPCHK(set_device(m->ctx->device));
        long long k = 0;
        if (components_label(m->ctx->stream, m->weld_inv.as<long long>(), m->weld_pts.as<double>(), nt, m->weld_n, &m->shells, &k, &m->shell_rounds, m->shell_ms)) return 1;
        m->n_shells = k;
        g_components_kernel_ms = m->shell_ms[0] + m->shell_ms[1];
    }
    out->n_shells = (int64_t)m->n_shells;
    out->rounds = (int64_t)m->shell_rounds;
    out->ms_label = m->shell_ms[0];
    out->ms_number = m->shell_ms[1];
    return 0;
}

int sdf_mesh_components_fetch(sdf_mesh *m, int32_t *h_vertex_shell, int32_t *h_triangle_shell, int64_t *h_triangles, int64_t *h_vertices,
                              double *h_bounds) {
    if (!m) { fail("sdf_mesh_components_fetch: NULL argument"); return 2; }
    if (m->n_shells < 0) { fail("sdf_mesh_components_fetch: call sdf_mesh_components first"); return 2; }
    if (m->n_shells == 0) return 0;
    static const char who[] = "sdf_mesh_components_fetch: ";
    sdf_ctx *c = m->ctx;
    const long long k = m->n_shells, nt = (long long)m->st.n_triangles;
    const ShellParts sp = shell_parts(m->shells.as<void>(), m->weld_n, nt, k);
    std::vector<unsigned long long> keys(h_bounds ? (size_t)(6 * k) : 0);
    HIPCHK(set_device(c->device));
    if (h_vertex_shell) HIPCHK_MSG(who, hipMemcpyAsync(h_vertex_shell, sp.vertex_shell, (size_t)m->weld_n * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_triangle_shell) HIPCHK_MSG(who, hipMemcpyAsync(h_triangle_shell, sp.triangle_shell, (size_t)nt * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_triangles) HIPCHK_MSG(who, hipMemcpyAsync(h_triangles, sp.triangles, (size_t)k * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_vertices) HIPCHK_MSG(who, hipMemcpyAsync(h_vertices, sp.vertices, (size_t)k * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_bounds) HIPCHK_MSG(who, hipMemcpyAsync(keys.data(), sp.box, (size_t)k * 48, hipMemcpyDeviceToHost, c->stream));
    const hipError_t e = stream_wait(c->stream);                      // (before `keys` goes, whatever the copies said)
    HIPCHK_MSG(who, e);
    if (h_bounds) shell_bounds(keys.data(), k, h_bounds);
    return 0;
}

int sdf_mesh_select_shells(sdf_mesh *m, const unsigned char *h_keep, int64_t n_keep, sdf_mesh **out) {
    if (!m || !out || (n_keep > 0 && !h_keep)) { fail("sdf_mesh_select_shells: NULL argument"); return 2; }
    *out = nullptr;
    if (m->n_shells < 0) { fail("sdf_mesh_select_shells: call sdf_mesh_components first"); return 2; }
    if (n_keep != (int64_t)m->n_shells) {
        fail("sdf_mesh_select_shells: the mask has " + std::to_string((long long)n_keep) + " entries, the mesh has " + std::to_string(m->n_shells) + " shells");
        return 2;
    }
    bool any = false;
    for (int64_t k = 0; k < n_keep; k++) any = any || h_keep[k] != 0;
    DevBuf soup;                                                       // the selection's own soup: the new mesh's `out`
    long long kept = 0;
    if (any) {                                                         // (keeping nothing: a mesh of 0 triangles, no launch)
        MESH_SOUP_READY(m);
        HIPCHK(set_device(m->ctx->device));
        const ShellParts sp = shell_parts(m->shells.as<void>(), m->weld_n, (long long)m->st.n_triangles, m->n_shells);
        if (components_select(m->ctx->stream, (const double *)mesh_soup(m), (long long)m->st.n_triangles, sp.triangle_shell, h_keep, m->n_shells,
                              &soup, &kept, &g_components_kernel_ms)) {
            soup.release();
            return 1;
        }
    }
    *out = derived_mesh(m, soup, (int64_t)kept);
    return 0;
}

double sdf_mesh_components_last_kernel_ms(void) { return g_components_kernel_ms; }

// ---- the mesh simplified: clusters of the welded vertices, quadric representatives, the survivors as a mesh of its own ----
static thread_local double g_simplify_kernel_ms[4] = {0.0, 0.0, 0.0, 0.0};

int sdf_mesh_simplify(sdf_mesh *m, const double *origin3, const double *cell3, double reg, sdf_mesh **out, sdf_simplify_stats *stats) {
    if (!m || !origin3 || !cell3 || !out || !stats) { fail("sdf_mesh_simplify: NULL argument"); return 2; }
    for (int k = 0; k < 3; k++) {
        if (!(std::isfinite(cell3[k]) && cell3[k] > 0.0)) { fail("sdf_mesh_simplify: cell must be positive and finite"); return 2; }
        if (!std::isfinite(origin3[k])) { fail("sdf_mesh_simplify: origin must be finite"); return 2; }
    }
    if (!(std::isfinite(reg) && reg >= 0.0)) { fail("sdf_mesh_simplify: reg must be finite and not negative"); return 2; }
    MESH_READY(m);
    const long long nt = (long long)m->st.n_triangles;
    if (3 * nt >= (1ll << 31)) { fail("sdf_mesh_simplify: 2^31 or more corners or vertices"); return 2; }
    *stats = sdf_simplify_stats();
    DevBuf soup;                                                       // the survivors' own soup: the new mesh's `out`
    if (nt > 0) {                                                      // (no triangles: a mesh of 0 triangles, no launch)
        int64_t nu = 0;
        if (sdf_mesh_weld(m, &nu)) return 1;
        HIPCHK(set_device(m->ctx->device));
        if (simplify_device(m->ctx->stream, m->weld_pts.as<double>(), m->weld_inv.as<long long>(), m->weld_n, nt, origin3, cell3, reg, &soup, stats, g_simplify_kernel_ms)) {
            soup.release();
            *stats = sdf_simplify_stats();
            return 1;
        }
    }
    *out = derived_mesh(m, soup, stats->triangles_out);
    return 0;
}

double sdf_mesh_simplify_last_kernel_ms(double *parts4) {
    for (int k = 0; parts4 && k < 4; k++) parts4[k] = g_simplify_kernel_ms[k];
    return g_simplify_kernel_ms[0] + g_simplify_kernel_ms[1] + g_simplify_kernel_ms[2] + g_simplify_kernel_ms[3];
}

// ---- the mesh simplified to a tolerance: the same clustering on the levels cell x 2^L, the coarsest accepted cluster per vertex ----
static thread_local double g_adaptive_kernel_ms[SDF_ADAPTIVE_MAX_LEVELS + 2] = {};     // the levels, then the emission
static thread_local int g_adaptive_levels = -1;

int sdf_mesh_simplify_adaptive(sdf_mesh *m, const double *origin3, const double *cell3, double reg, double tolerance, int levels,
                               sdf_mesh **out, sdf_adaptive_stats *stats) {
    if (!m || !origin3 || !cell3 || !out || !stats) { fail("sdf_mesh_simplify_adaptive: NULL argument"); return 2; }
    if (levels < 0 || levels > SDF_ADAPTIVE_MAX_LEVELS) { fail("sdf_mesh_simplify_adaptive: levels must lie in 0 .. 10"); return 2; }
    if (!(tolerance >= 0.0)) { fail("sdf_mesh_simplify_adaptive: tolerance must not be negative or NaN"); return 2; }
    for (int k = 0; k < 3; k++) {
        if (!(std::isfinite(cell3[k]) && cell3[k] > 0.0)) { fail("sdf_mesh_simplify_adaptive: cell must be positive and finite"); return 2; }
        if (!std::isfinite(cell3[k] * (double)(1 << levels))) { fail("sdf_mesh_simplify_adaptive: cell x 2^levels must be finite"); return 2; }
        if (!std::isfinite(origin3[k])) { fail("sdf_mesh_simplify_adaptive: origin must be finite"); return 2; }
    }
    if (!(std::isfinite(reg) && reg >= 0.0)) { fail("sdf_mesh_simplify_adaptive: reg must be finite and not negative"); return 2; }
    MESH_READY(m);
    const long long nt = (long long)m->st.n_triangles;
    if (3 * nt >= (1ll << 31)) { fail("sdf_mesh_simplify_adaptive: 2^31 or more corners or vertices"); return 2; }
    *stats = sdf_adaptive_stats();
    stats->levels = levels;
    DevBuf soup;                                                       // the survivors' own soup: the new mesh's `out`
    if (nt > 0) {                                                      // (no triangles: a mesh of 0 triangles, no launch)
        int64_t nu = 0;
        if (sdf_mesh_weld(m, &nu)) return 1;
        HIPCHK(set_device(m->ctx->device));
        for (double &ms : g_adaptive_kernel_ms) ms = 0.0;
        g_adaptive_levels = levels;
        if (simplify_adaptive_device(m->ctx->stream, m->weld_pts.as<double>(), m->weld_inv.as<long long>(), m->weld_n, nt, origin3, cell3, reg,
                                     tolerance, levels, &soup, stats, g_adaptive_kernel_ms, &g_adaptive_kernel_ms[levels + 1])) {
            soup.release();
            *stats = sdf_adaptive_stats();
            return 1;
        }
    }
    *out = derived_mesh(m, soup, stats->triangles_out);
    return 0;
}

double sdf_mesh_simplify_adaptive_last_kernel_ms(double *ms) {
    double total = 0.0;
    for (int k = 0; k <= g_adaptive_levels + 1; k++) {
        if (ms && k <= g_adaptive_levels) ms[k] = g_adaptive_kernel_ms[k];
        total += g_adaptive_kernel_ms[k];
    }
    return total;
}

// ---- the mesh mended: duplicate triangles dropped, oppositely wound pairs cancelled, the survivors as a mesh of its own ----
static thread_local double g_mend_kernel_ms[3] = {0.0, 0.0, 0.0};

int sdf_mesh_mend(sdf_mesh *m, sdf_mesh **out, sdf_mend_stats *stats) {
    if (!m || !out || !stats) { fail("sdf_mesh_mend: NULL argument"); return 2; }
    MESH_READY(m);
    const long long nt = (long long)m->st.n_triangles;
    if (3 * nt >= (1ll << 31)) { fail("sdf_mesh_mend: 2^31 or more corners or vertices"); return 2; }      // (a weld has no more vertices than corners)
    *stats = sdf_mend_stats();
    DevBuf soup;                                                       // the survivors' own soup: the new mesh's `out`
    if (nt > 0) {                                                      // (no triangles: a mesh of 0 triangles, no launch)
        int64_t nu = 0;
        if (sdf_mesh_weld(m, &nu)) return 1;                           // (it also makes the float64 soup of a records mesh)
        HIPCHK(set_device(m->ctx->device));
        if (mend_device(m->ctx->stream, (const double *)mesh_soup(m), m->weld_inv.as<long long>(), m->weld_n, nt, &soup, stats, g_mend_kernel_ms)) {
            soup.release();
            *stats = sdf_mend_stats();
            return 1;
        }
    }
    *out = derived_mesh(m, soup, stats->triangles_out);
    return 0;
}

double sdf_mesh_mend_last_kernel_ms(double *parts3) {
    for (int k = 0; parts3 && k < 3; k++) parts3[k] = g_mend_kernel_ms[k];
    return g_mend_kernel_ms[0] + g_mend_kernel_ms[1] + g_mend_kernel_ms[2];
}

// ---- build directions rated: extents, overhang and bed-contact totals per direction, classes per triangle ----
static thread_local double g_overhang_kernel_ms = 0.0;
static thread_local long long g_overhang_slabs = 0;

int sdf_mesh_overhangs(sdf_mesh *m, const double *h_dirs, int64_t n_dirs, double sin_limit, double bed_tol, size_t max_scratch_bytes,
                       double *h_values, int64_t *h_counts) {
    if (!m || !h_dirs || !h_values || !h_counts) { fail("sdf_mesh_overhangs: NULL argument"); return 2; }
    if (overhang_refused("sdf_mesh_overhangs", h_dirs, (long long)n_dirs, sin_limit, bed_tol)) return 2;
    MESH_READY(m);
    if ((long long)m->st.n_triangles >= (1ll << 31)) { fail("sdf_mesh_overhangs: 2^31 or more triangles"); return 2; }
    g_overhang_kernel_ms = 0.0;
    g_overhang_slabs = 0;
    for (int64_t k = 0; k < n_dirs; k++) {                             // the empty result: no launch for a mesh of 0 triangles
        h_values[5 * k] = INFINITY; h_values[5 * k + 1] = -INFINITY;
        h_values[5 * k + 2] = h_values[5 * k + 3] = h_values[5 * k + 4] = 0.0;
        h_counts[2 * k] = h_counts[2 * k + 1] = 0;
    }
    if (m->st.n_triangles == 0) return 0;
    MESH_SOUP_READY(m);
    HIPCHK(set_device(m->ctx->device));
    return overhang_rate(m->ctx->stream, (const double *)mesh_soup(m), (long long)m->st.n_triangles, h_dirs, (long long)n_dirs, sin_limit,
                         bed_tol, max_scratch_bytes, h_values, h_counts, &g_overhang_slabs, &g_overhang_kernel_ms);
}

int sdf_mesh_overhang_classes(sdf_mesh *m, const double *h_dir3, double sin_limit, double bed_tol, uint8_t *h_classes) {
    if (!m || !h_dir3 || !h_classes) { fail("sdf_mesh_overhang_classes: NULL argument"); return 2; }
    if (overhang_refused("sdf_mesh_overhang_classes", h_dir3, 1, sin_limit, bed_tol)) return 2;
    MESH_READY(m);
    if ((long long)m->st.n_triangles >= (1ll << 31)) { fail("sdf_mesh_overhang_classes: 2^31 or more triangles"); return 2; }
    g_overhang_kernel_ms = 0.0;
    g_overhang_slabs = 0;
    if (m->st.n_triangles == 0) return 0;
    MESH_SOUP_READY(m);
    HIPCHK(set_device(m->ctx->device));
    return overhang_classes(m->ctx->stream, (const double *)mesh_soup(m), (long long)m->st.n_triangles, h_dir3, sin_limit, bed_tol, h_classes,
                            &g_overhang_kernel_ms);
}

double sdf_overhang_last_kernel_ms(int64_t *n_slabs) {
    if (n_slabs) *n_slabs = (int64_t)g_overhang_slabs;
    return g_overhang_kernel_ms;
}

// ---- the indexed export: binary PLY records of the welded mesh, with the field normals that sdf_mesh_vertex_normals left ----
int sdf_mesh_emit_ply_host(sdf_mesh *m, int with_normals, void *h_vertices, void *h_faces) {
    if (!m || !h_vertices || !h_faces) { fail("sdf_mesh_emit_ply_host: NULL argument"); return 2; }
    if (m->weld_n < 0) { fail("sdf_mesh_emit_ply_host: call sdf_mesh_weld first"); return 2; }
    if (with_normals && !m->nrm_valid) { fail("sdf_mesh_emit_ply_host: with_normals needs a successful sdf_mesh_vertex_normals first"); return 2; }
    const long long nu = m->weld_n, nt = (long long)m->st.n_triangles;
    if (nu >= (1ll << 31)) { fail("sdf_mesh_emit_ply_host: 2^31 or more vertices: the face records hold 32-bit indices"); return 2; }
    if (nu == 0 || nt == 0) return 0;
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    const int width = with_normals ? 6 : 3;
    const long long nfl = nu * width;
    const size_t vbytes = (size_t)nfl * 4, fbytes = (size_t)nt * 13;
    float *verts;
    unsigned char *faces;
    Scratch scratch(c->stream);
    scratch.part(&verts, (size_t)nfl);
    scratch.part(&faces, fbytes);
    HIPCHK_MSG("sdf_mesh_emit_ply_host: hipMalloc(" + std::to_string(align256(vbytes) + fbytes) + "): ", scratch.alloc());
    static const char who[] = "sdf_mesh_emit_ply_host: ";
    launch_k_ply_vertices(dim3((unsigned)((nfl + 255) / 256)), dim3(256), c->stream, m->weld_pts.as<double>(), with_normals ? m->nrm.as<double>() : nullptr, nfl, width, verts);
    HIPCHK_MSG(who, hipGetLastError());
    launch_k_ply_faces(dim3((unsigned)((nt + 255) / 256)), dim3(256), c->stream, m->weld_inv.as<long long>(), nt, faces);
    HIPCHK_MSG(who, hipGetLastError());
    HIPCHK_MSG(who, hipMemcpyAsync(h_vertices, verts, vbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_MSG(who, hipMemcpyAsync(h_faces, faces, fbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_MSG(who, stream_wait(c->stream));
    return 0;
}

int sdf_mesh_kinds(sdf_mesh *m, uint8_t *h_out) {
    if (!m || !h_out) return fail("sdf_mesh_kinds: NULL argument");
    MESH_READY(m);
    if (m->st.n_batches == 0) return 0;
    HIPCHK(set_device(m->ctx->device));
    HIPCHK(hipMemcpyAsync(h_out, m->kinds.p, (size_t)m->st.n_batches, hipMemcpyDeviceToHost, m->ctx->stream));
    HIPCHK(stream_wait(m->ctx->stream));
    for (int64_t i = 0; i < m->st.n_batches; i++) if (h_out[i] == 255) h_out[i] = 3;
    return 0;
}

int sdf_mesh_prune_masks(sdf_mesh *m, uint32_t *h_out) {
    if (!m || !h_out) return fail("sdf_mesh_prune_masks: NULL argument");
    MESH_READY(m);
    if (!m->pruned) return fail("sdf_mesh_prune_masks: this mesh was generated without the interval prepass");
    const size_t n = (size_t)m->st.n_batches;
    if (n == 0) return 0;
    HIPCHK(set_device(m->ctx->device));
    HIPCHK(hipMemcpyAsync(h_out, m->prune.p, n * 64, hipMemcpyDeviceToHost, m->ctx->stream));
    HIPCHK(stream_wait(m->ctx->stream));
    return 0;
}

int sdf_mesh_destroy(sdf_mesh *m) {
    if (!m) return 0;
    sdf_ctx *c = m->ctx;
    (void)hipSetDevice(c->device);
    (void)stream_wait(c->stream);
    if (m->stream) (void)stream_wait(m->stream);        // (a call slot's lane)
    if (m->pend.active) { c->slots[m->pend.got.slot].busy = false; c->slots[m->pend.got.slot].owner = nullptr; m->pend.active = false; }   // (abandoned; the stream is idle now)
    if (m->out.p) {   // keep one soup buffer around for the next call
        if (c->arena_pool.empty()) c->arena_pool.push_back(m->out);
        else if (c->arena_pool.back().bytes < m->out.bytes) { c->arena_pool.back().release(); c->arena_pool.back() = m->out; }
        else m->out.release();
        m->out.p = nullptr; m->out.bytes = 0;
    }
    if (m->counters.p) { c->counter_pool.push_back(m->counters); m->counters.p = nullptr; m->counters.bytes = 0; }
    for (DevBuf *b : {&m->axes, &m->kinds, &m->worklist, &m->status, &m->prune, &m->tapes, &m->cull, &m->order, &m->desc, &m->cellrecs, &m->trilist, &m->blockidx, &m->slab}) b->release();
    delete m;
    return 0;
}

}  // extern "C"
