// sdf_chunked.hip -- meshing a grid through device memory, a chunk of batches per submission: `generate` for batch_size > 32
// (generate_big: the tape samples the tiles, k_eval_tiles) and for models with user closures at any batch size (sdf_generate_field:
// a host callback samples them).  One driver, march_chunks, with a sampler per path; the arithmetic the GPU never sees is
// sdf_chunk_plan.h.  Host code only: it launches through the launchers of sdf_plain.h and through enqueue_skip (sdf_prepass.hip) /
// enqueue_eval_tiles (sdf_eval.hip), so it is built WITHOUT the interpreters' structurizer option (build.units).
#include <algorithm>
#include <cmath>

#include "sdf_internal.h"
#include "sdf_plain.h"

using namespace sdfk;

// the tile of a batch at sample vol_off of a chunk's volume buffer
static FieldTile field_tile(const double *X, const double *Y, const double *Z, const BatchBox &o, size_t vol_off) {
    FieldTile tl;
    tl.vol_off = (long long)vol_off; tl.n0 = o.lx; tl.n1 = o.ly; tl.n2 = o.lz; tl.pad_ = 0;
    // scale = the batch's first axis step (reference sdf/core.py:58-59: `X[1] - X[0]` of the batch's slices);
    // a one-sample axis has none and the tile has no cells, so its value is never used
    tl.of[0] = X[o.ox]; tl.of[1] = Y[o.oy]; tl.of[2] = Z[o.oz];
    tl.sc[0] = o.lx > 1 ? X[o.ox + 1] - X[o.ox] : 0.0; tl.sc[1] = o.ly > 1 ? Y[o.oy + 1] - Y[o.oy] : 0.0; tl.sc[2] = o.lz > 1 ? Z[o.oz + 1] - Z[o.oz] : 0.0;
    return tl;
}

// One chunk of nt <= FIELD_CHUNK_MAX tiles whose float32 volumes (the context's field_vol) and FieldTile table (field_tiles) are
// on the device, marched into the ordered soup behind its first `total` triangles: k_field_rows / k_scan_rows number the
// triangles and count the ambiguous cells, the host reads the offsets and classifies the chunk's `batches` (kinds 1 = empty,
// 2 = non-empty), the soup grows, k_field_emit writes `points * scale + offset`; waits for the chunk.  prefix (or NULL): per tile its inclusive
// triangle prefix as a look-back word of the fused path.
static int march_chunk(sdf_mesh *m, hipStream_t st, const int *batches, int nt, int slots, uint8_t *kinds, unsigned long long &total,
                       unsigned long long *prefix) {
    sdf_ctx *c = m->ctx;
    const size_t nslots = (size_t)nt * slots;
    // (behind the nslots row offsets: the chunk's triangle total, then its count of ambiguous cells)
    unsigned long long *d_total = (unsigned long long *)c->rows_off.p + nslots;
    HIPCHK(hipMemsetAsync(d_total + 1, 0, 8, st));
    launch_k_field_rows(dim3((unsigned)(slots / 256), (unsigned)nt), dim3(256), st, (const McTables *)c->mc.p, (const float *)c->field_vol.p,
                        (const FieldTile *)c->field_tiles.p, (unsigned *)c->rows.p, slots, d_total + 1);
    launch_k_scan_rows(dim3(1), dim3(1024), st, (const unsigned *)c->rows.p, (long long)nslots, (unsigned long long *)c->rows_off.p, d_total);
    HIPCHK(hipGetLastError());
    // (per tile only its first slot's offset, the chunk's total and its ambiguous cells are needed on the host)
    unsigned long long offs[FIELD_CHUNK_MAX + 2];
    HIPCHK(hipMemcpy2DAsync(offs, 8, c->rows_off.p, (size_t)slots * 8, 8, (size_t)nt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&offs[nt], d_total, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    const unsigned long long chunk_total = offs[nt];
    m->st.n_ambiguous_cells += (int64_t)offs[nt + 1];
    for (int j = 0; j < nt; j++) {
        const unsigned long long cnt = offs[j + 1] - offs[j];
        kinds[(size_t)batches[j]] = cnt ? 2 : 1;
        if (cnt) m->st.n_nonempty++; else m->st.n_empty++;
        if (prefix) prefix[j] = MESH_FLAG_PFX | (total + offs[j + 1]);
    }
    if (!chunk_total) return 0;
    if (const size_t grown = soup_growth(m->out.bytes, total, chunk_total)) {   // grow the soup (geometric), keeping what is there
        DevBuf bigger;
        if (bigger.ensure(grown)) return 1;
        if (total) HIPCHK(hipMemcpyAsync(bigger.p, m->out.p, (size_t)total * 72, hipMemcpyDeviceToDevice, st));
        HIPCHK(stream_wait(st));
        m->out.release();
        m->out = bigger;
    }
    launch_k_field_emit(dim3((unsigned)(slots / 256), (unsigned)nt), dim3(256), st, (const McTables *)c->mc.p, (const float *)c->field_vol.p,
                        (const FieldTile *)c->field_tiles.p, (const unsigned long long *)c->rows_off.p, (double *)m->out.p, total,
                        (unsigned long long)(m->out.bytes / 72), slots);
    HIPCHK(hipGetLastError());
    HIPCHK(stream_wait(st));   // (the chunk's buffers are refilled next)
    total += chunk_total;
    return 0;
}

// The batch loop of both paths: items [w_begin, w_end) of the work list, plan.ch at a time.  Per chunk it builds the tiles,
// `sample(tiles, boxes, nt, npts)` puts their float32 volumes (npts samples, tile after tile) and the tile table on the device --
// the one thing the paths do differently -- and march_chunk meshes them.  Then the statistics of the whole call, the verdicts
// back on the device (work items of other shards stay 255 = "other shard", like the fused path) and one wait.  The tape path also
// keeps, per work item, its inclusive triangle prefix as a look-back word of the fused path (`prefix`, else NULL), so that
// sdf_mesh_batch_offsets serves its meshes too, and an event behind the last chunk (`marched`, else NULL).
template <typename Sampler>
static int march_chunks(sdf_mesh *m, hipStream_t st, const double *X, const double *Y, const double *Z, const int *work, int w_begin, int w_end,
                        uint8_t *kinds, const ChunkPlan &plan, unsigned long long *prefix, hipEvent_t marched, Sampler sample) {
    const GridDesc &g = m->g;
    const size_t nb = (size_t)m->st.n_batches;
    std::vector<FieldTile> tiles((size_t)plan.ch);
    std::vector<BatchBox> boxes((size_t)plan.ch);
    unsigned long long total = 0;
    for (int w0 = w_begin; w0 < w_end; w0 += plan.ch) {
        const int nt = std::min(plan.ch, w_end - w0);
        size_t npts = 0;
        for (int j = 0; j < nt; j++) {
            const BatchBox o = boxes[(size_t)j] = batch_box(g.nx, g.ny, g.nz, g.bs, work[w0 + j]);
            tiles[(size_t)j] = field_tile(X, Y, Z, o, npts);
            npts += (size_t)o.lx * o.ly * o.lz;
        }
        m->st.n_eval_voxels += (int64_t)npts;
        if (sample(tiles.data(), boxes.data(), nt, npts)) return 1;
        if (march_chunk(m, st, work + w0, nt, plan.slots, kinds, total, prefix ? prefix + (w0 - w_begin) : nullptr)) return 1;
    }
    if (marched) HIPCHK(hipEventRecord(marched, st));
    m->st.n_triangles = (int64_t)total;
    m->st.n_sampled_voxels = m->st.n_eval_voxels;
    if (m->kinds.ensure(nb)) return 1;
    HIPCHK(hipMemcpyAsync(m->kinds.p, kinds, nb, hipMemcpyHostToDevice, st));
    if (prefix && w_end > w_begin)
        HIPCHK(hipMemcpyAsync((unsigned long long *)m->status.p + w_begin, prefix, (size_t)(w_end - w_begin) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(stream_wait(st));
    return 0;
}

// `generate` for batch_size > 32 (reference sdf/core.py:87, 114-119 takes any batch size): the (batch_size + 1)^3 float32 tile
// of such a batch does not fit the LDS of a compute unit (33^3 = 144 KB of 160 KB does), so the fused kernels do not apply.  The
// batches go through device memory instead, a chunk of them per submission: k_eval_tiles samples the chunk's tiles into float32
// volumes (the interpreter, a lane per sample), k_field_rows / k_scan_rows / k_field_emit march them and write
// `points * scale + offset` into the ordered float64 soup -- the kernels behind sdf_generate_field, with the tape instead of a
// host callback.  The skip test is k_skip's, the work list k_compact's.  One host synchronisation per chunk: a chunk is
// >= 2.7e5 samples per batch, the launches are long.  Synchronous; the soup lives in library memory.
int generate_big(sdf_mesh *m, const GenCall &call) {
    sdf_tape *t = call.tape;
    sdf_ctx *c = t->ctx;
    hipStream_t st = c->stream;
    const int nx = call.nx, ny = call.ny, nz = call.nz, bs = call.bs;
    GridDesc &g = m->g;
    int nb = 0;
    if (grid_batches(nx, ny, nz, bs, "sdf_generate", g, nb)) return 1;
    m->st.n_batches = nb;
    m->st.n_grid_voxels = (int64_t)nx * ny * nz;
    if (nb == 0) return 0;
    if (m->axes.ensure((size_t)(nx + ny + nz) * 8) || m->kinds.ensure((size_t)nb) || m->worklist.ensure((size_t)nb * 4) ||
        m->status.ensure((size_t)nb * 8) || m->counters.ensure(sizeof(MeshCounters)))
        return 1;
    double *dX = (double *)m->axes.p, *dY = dX + nx, *dZ = dY + ny;
    g.X = dX; g.Y = dY; g.Z = dZ;
    HIPCHK(hipEventRecord(c->ev[0], st));
    HIPCHK(hipMemcpyAsync(dX, call.X, (size_t)nx * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dY, call.Y, (size_t)ny * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dZ, call.Z, (size_t)nz * 8, hipMemcpyHostToDevice, st));
    if (call.sparse) { if (enqueue_skip(t, dX, nx, ny, nz, bs, 0, nb, call.precision, (unsigned char *)m->kinds.p, st)) return 1; }
    else HIPCHK(hipMemsetAsync(m->kinds.p, 255, (size_t)nb, st));
    launch_k_compact(dim3(1), dim3(1024), st, (const unsigned char *)m->kinds.p, nb, (int *)m->worklist.p, (MeshCounters *)m->counters.p,
                     (unsigned long long *)m->status.p, (long long)call.shard_index, (long long)call.shard_count);
    HIPCHK(hipGetLastError());
    MeshCounters h;
    HIPCHK(hipMemcpyAsync(&h, m->counters.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    std::vector<int> work((size_t)std::max(h.nwork, 1));
    if (h.nwork) HIPCHK(hipMemcpy(work.data(), m->worklist.p, (size_t)h.nwork * 4, hipMemcpyDeviceToHost));
    std::vector<uint8_t> kinds((size_t)nb);
    HIPCHK(hipMemcpy(kinds.data(), m->kinds.p, (size_t)nb, hipMemcpyDeviceToHost));
    HIPCHK(hipEventRecord(c->ev[1], st));
    m->work_begin = h.work_begin; m->work_end = h.work_end;
    m->st.n_skipped = nb - h.nwork;
    m->st.n_work_begin = h.work_begin; m->st.n_work_end = h.work_end;

    const ChunkPlan plan = chunk_plan(bs, false);
    if (c->field_vol.ensure((size_t)plan.ch * plan.tile * 4) || c->field_tiles.ensure(sizeof(FieldTile) * plan.ch + (size_t)plan.ch * 12) ||
        c->rows.ensure((size_t)plan.ch * plan.slots * 4) || c->rows_off.ensure(((size_t)plan.ch * plan.slots + 2) * 8))
        return 1;
    int *d_org = reinterpret_cast<int *>((char *)c->field_tiles.p + sizeof(FieldTile) * plan.ch);   // behind the tile table: a tile's first sample per axis
    std::vector<int> org((size_t)plan.ch * 3);
    std::vector<unsigned long long> prefix((size_t)std::max(h.work_end - h.work_begin, 1));
    auto sample = [&](const FieldTile *tiles, const BatchBox *boxes, int nt, size_t) -> int {
        size_t big = 0;
        for (int j = 0; j < nt; j++) {
            org[(size_t)3 * j] = boxes[j].ox; org[(size_t)3 * j + 1] = boxes[j].oy; org[(size_t)3 * j + 2] = boxes[j].oz;
            big = std::max(big, (size_t)tiles[j].n0 * tiles[j].n1 * tiles[j].n2);
        }
        HIPCHK(hipMemcpyAsync(c->field_tiles.p, tiles, sizeof(FieldTile) * (size_t)nt, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_org, org.data(), (size_t)nt * 12, hipMemcpyHostToDevice, st));
        enqueue_eval_tiles(t, call.precision, dX, dY, dZ, (const FieldTile *)c->field_tiles.p, d_org, (float *)c->field_vol.p, big, nt, st);
        return 0;
    };
    if (march_chunks(m, st, call.X, call.Y, call.Z, work.data(), h.work_begin, h.work_end, kinds.data(), plan, prefix.data(), c->ev[2], sample))
        return 1;
    m->st.n_batch_instrs = (int64_t)(t->n_words / 2 - 1) * (h.work_end - h.work_begin);
    float ms_pre = 0, ms_tot = 0;
    HIPCHK(hipEventElapsedTime(&ms_pre, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&ms_tot, c->ev[0], c->ev[2]));
    m->st.ms_prepass = ms_pre; m->st.ms_total = ms_tot; m->st.ms_mesh = ms_tot - ms_pre;
    m->emitted_to = nullptr;
    return 0;
}

extern "C" {

// The batch loop of `generate` (reference sdf/core.py:114-141) around a field that lives on the HOST: a user-written
// closure (reference README.md:258-295, sdf/d3.py:48-63), possibly calling device-resident sub-models itself.  The
// library does what the reference's `_skip` / `_worker` do around `sdf(P)`: it builds the points of the skip test and
// of every surviving batch (`_cartesian_product`, first axis slowest), hands them to the callback, and meshes the
// returned values on the device -- a chunk of batches per submission: float32 cast, marching cubes of all tiles,
// one scan for the order, `points * scale + offset` into the ordered float64 soup.
int sdf_generate_field(sdf_ctx *c, sdf_field_fn field, void *user, const double *X, int nx, const double *Y, int ny,
                       const double *Z, int nz, int bs, int sparse, int64_t shard_index, int64_t shard_count, sdf_mesh **out) {
    if (!c || !field || !X || !Y || !Z || !out) return fail("sdf_generate_field: NULL argument");
    *out = nullptr;
    if (bs < 1 || bs > SDF_BATCH_SIZE_MAX) return fail("sdf_generate_field: batch_size must be in 1..512");
    if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return fail("sdf_generate_field: bad shard");
    if (nx < 0 || ny < 0 || nz < 0) return fail("sdf_generate_field: negative axis length");
    HIPCHK(set_device(c->device));
    sdf_mesh *m = new sdf_mesh();
    m->ctx = c;
    void *h_pts = nullptr, *h_vals = nullptr;
    struct Guard {
        sdf_mesh *&m; void *&a; void *&b;
        ~Guard() { const std::string keep = g_err; if (a) sdf_host_free(a); if (b) sdf_host_free(b); if (m) sdf_mesh_destroy(m); g_err = keep; }
    } guard{m, h_pts, h_vals};
    GridDesc &g = m->g;
    int nb = 0;
    if (grid_batches(nx, ny, nz, bs, "sdf_generate_field", g, nb)) return 1;
    m->st.n_batches = nb;
    m->st.n_grid_voxels = (int64_t)nx * ny * nz;
    if (nb == 0) { *out = m; m = nullptr; return 0; }
    const ChunkPlan plan = chunk_plan(bs, true);
    // points per callback: a chunk's, <= 64 M = 2 GB of pinned points + values -- except that ONE tile is always taken whole:
    // (512 + 1)^3 points = 4.3 GB at the largest batch size
    const size_t pts_cap = std::max<size_t>((size_t)plan.ch * plan.tile, (size_t)9 << 12);
    if (sdf_host_alloc(pts_cap * 24, &h_pts) || sdf_host_alloc(pts_cap * 8, &h_vals)) return 1;
    double *pts = (double *)h_pts, *vals = (double *)h_vals;
    std::vector<uint8_t> kinds((size_t)nb, 255);

    // ---- `_skip` (reference sdf/core.py:28-43): centre + the 8 corners of every batch through the field ----
    if (sparse) {
        const int per = (int)(pts_cap / 9);
        for (int b0 = 0; b0 < nb; b0 += per) {
            const int n = std::min(per, nb - b0);
            for (int j = 0; j < n; j++) {
                const BatchBox o = batch_box(nx, ny, nz, bs, b0 + j);
                skip_points(X[o.ox], X[o.ox + o.lx - 1], Y[o.oy], Y[o.oy + o.ly - 1], Z[o.oz], Z[o.oz + o.lz - 1], pts + (size_t)j * 27);
            }
            if (field(user, pts, (int64_t)n * 9, vals)) return fail("sdf_generate_field: the field callback failed");
            for (int j = 0; j < n; j++) kinds[(size_t)(b0 + j)] = skip_verdict(pts + (size_t)j * 27, vals + (size_t)j * 9);
        }
    }
    std::vector<int> work;
    for (int b = 0; b < nb; b++) if (kinds[(size_t)b]) work.push_back(b);
    const long long nwork = (long long)work.size();
    const int w_begin = shard_cut(nwork, shard_index, shard_count), w_end = shard_cut(nwork, shard_index + 1, shard_count);
    m->work_begin = w_begin; m->work_end = w_end;
    m->st.n_skipped = nb - (int64_t)nwork;
    m->st.n_work_begin = w_begin; m->st.n_work_end = w_end;

    // ---- `_worker` for the shard's batches: the chunk's points through the field, its values cast to float32 on the device ----
    auto sample = [&](const FieldTile *tiles, const BatchBox *boxes, int nt, size_t npts) -> int {
        for (int j = 0; j < nt; j++) {
            const BatchBox &o = boxes[j];
            double *p = pts + (size_t)tiles[j].vol_off * 3;
            for (int ix = 0; ix < o.lx; ix++)
                for (int iy = 0; iy < o.ly; iy++)
                    for (int iz = 0; iz < o.lz; iz++, p += 3) { p[0] = X[o.ox + ix]; p[1] = Y[o.oy + iy]; p[2] = Z[o.oz + iz]; }
        }
        if (field(user, pts, (int64_t)npts, vals)) return fail("sdf_generate_field: the field callback failed");
        const size_t nslots = (size_t)nt * plan.slots;
        if (c->field_vals.ensure(npts * 8) || c->field_vol.ensure(npts * 4) || c->field_tiles.ensure(sizeof(FieldTile) * plan.ch) ||
            c->rows.ensure(nslots * 4) || c->rows_off.ensure((nslots + 2) * 8))
            return 1;
        HIPCHK(hipMemcpyAsync(c->field_vals.p, vals, npts * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->field_tiles.p, tiles, sizeof(FieldTile) * (size_t)nt, hipMemcpyHostToDevice, c->stream));
        launch_k_cast_f32(dim3((unsigned)((npts + 255) / 256)), dim3(256), c->stream, (const double *)c->field_vals.p,
                          (float *)c->field_vol.p, (long long)npts);
        return 0;
    };
    // (no look-back words: sdf_mesh_batch_offsets refuses these meshes)
    if (march_chunks(m, c->stream, X, Y, Z, work.data(), w_begin, w_end, kinds.data(), plan, nullptr, nullptr, sample)) return 1;
    *out = m;
    m = nullptr;
    return 0;
}

}  // extern "C"
