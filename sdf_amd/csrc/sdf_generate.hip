// sdf_generate.hip -- the generate pipeline of libsdf_hip.so's C ABI (gfx950 only): one call descriptor (GenCall, sdf_internal.h) from the
// entry points sdf_generate* through a call slot, the axes' staging, the prepass, the meshing attempts and the statistics, to a mesh
// handle.  The rest of the ABI: sdf_ctx.hip (contexts, tapes), sdf_eval.hip, sdf_runtime.hip, sdf_chunked.hip, sdf_mesh_out.hip, sdf_probe_out.hip,
// sdf_comm.hip and the features' own units.
//
// Host code only: it launches through enqueue_prepass / enqueue_cull (sdf_prepass.hip), the k_mesh launchers of sdf_mesh_inst.hip and
// the launchers of sdf_plain.h, like sdf_chunked.hip and sdf_comm.hip, which drive it.  So the unit takes the plain flags, WITHOUT the
// interpreters' structurizer option (build.units), and a change to the pipeline recompiles no interpreter.
//
// Kernels of the library (one call of sdf_generate enqueues k_skip -> k_compact [-> k_prune_list] -> k_cull -> k_mesh
// [-> k_scan_items -> k_emit2] on one stream, without a host round trip in between)
//   k_eval_points / k_eval_grid   f(P): the tape interpreter alone; k_eval_points_ext: with user closures (L_EXTERN) (sdf_eval.hip)
//   k_eval_tiles                  the float32 volumes of a chunk of batches of more than 33^3 samples (batch_size > 32: generate_big,
//                                 sdf_chunked.hip) (sdf_eval.hip)
//   k_estimate_bounds_w           the reference's `_estimate_bounds` loop (sdf/core.py:62-82) as one launch (sdf_bounds.hip)
//   k_skip / k_skip_rare          the reference's `_skip` predicate for every batch at once
//                                 (reference sdf/core.py:28-43), 9 lanes per batch, 7 batches per wave; its surplus
//                                 workgroups run the interval pruning pass of the same batches (sdf_prune.h) (sdf_prepass.hip)
//   k_compact                     ordered work list of the surviving batches; clears the counters / look-back words (sdf_plain.hip)
//   k_prune_list                  the pruning pass for the survivors only (grids with many batches) (sdf_prepass.hip)
//   k_cull / k_cull_lean          per surviving batch: the sampling tasks that have to be evaluated, by interval
//                                 arithmetic over groups of 4^3 cells (cull_tasks, sdf_device.h) (sdf_prepass.hip)
//   k_mesh (sdf_device.h)         THE hot kernel: one persistent workgroup per CU pulls batches
//                                 from the work list; samples the (<=33)^3 tile through the tape
//                                 interpreter (float64 -> float32 like skimage's cast) straight
//                                 into LDS (143,748 B of gfx950's 160 KiB), classifies the cells,
//                                 finds the batch's place in the ordered soup by a look-back over
//                                 the earlier batches' counts and writes the float64 world-space
//                                 triangles in reference order (reference `_worker`,
//                                 sdf/core.py:45-60, and `points.extend`, :141) (instantiated in sdf_mesh_inst.hip)
//   k_scan_items / k_emit2        two-pass meshing (long tapes): k_mesh stops at the classification, these number
//                                 and write the triangles (sdf_plain.hip, like the following up to k_ply_*)
//   k_pack_slab / k_expand        multi-GPU exchange: a shard's soup as a fixed-capacity slab / the gathered slabs
//                                 expanded into the ordered float64 soup; k_collect_headers: the slabs' heads for the host
//   k_mc_rows / k_scan_rows / k_mc_emit   marching cubes of a caller-supplied volume (`_marching_cubes`);
//   k_cast_f32 / k_field_*        the same for the chunks of batches that go through device memory (sdf_chunked.hip: a
//                                 host-evaluated field = user closures, and batch_size > 32)
//   k_stl                         50-byte STL records (reference sdf/stl.py:4-24); k_ply_vertices / k_ply_faces: binary PLY records
//   k_vertex_normals              the field's gradient at the welded vertices (sdf_normals.hip)
//   k_render                      sphere tracing of a model: depth, normals, steps per pixel (sdf_render.hip)
//   k_vertex_thickness            the wall thickness at the welded vertices: inward rays through the field (sdf_thickness.hip)
//   k_weld_*                      a soup's unique vertices and the index of every row (sdf_weld.hip)
//   k_ls_*                        a mesh as a level set: distances, parity / winding signs, composition (sdf_level_set.hip)
//   k_edt_*                       the exact Euclidean distance transform of `text` / `image` (sdf_edt.hip)
//   k_soup_* / k_moment_partials / k_edge_*   volume, area, inertia and the edge census of a mesh (sdf_measure.hip)
//   k_shell_* / k_keep_flags / k_select_copy   the connected shells of a mesh and their selection (sdf_components.hip)
//   k_cluster_* / k_item_starts / k_adaptive_*   a mesh simplified by vertex clustering with quadric vertices, on one grid or to a tolerance (sdf_simplify.hip)
//   k_mend_*                      a mesh mended: duplicate triangles dropped, opposite pairs cancelled (sdf_mend.hip)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "sdf_plain.h"
#include "sdf_internal.h"

using namespace sdfk;

// the grid of a call (grid_desc, sdf_internal.h) for an entry point that indexes the batches with an int (`who` names it in the message)
int grid_batches(int nx, int ny, int nz, int bs, const char *who, GridDesc &g, int &nb) {
    const long long nb64 = grid_desc(nx, ny, nz, bs, g);
    if (nb64 > 0x7fffffffLL) return fail(std::string(who) + ": too many batches");
    nb = (int)nb64;
    return 0;
}

// k_mesh's dynamic LDS behind the fixed part: the float32 tile, the sign bits, the list region (which also receives the
// batch's cull record) -- launch_mesh passes the layout to the kernel, generate_impl asks it whether a cull record fits
struct MeshLds { size_t bits_off, list_off, list_cap; };
static MeshLds mesh_lds(int bs, size_t lds_max) {
    const size_t nvox = (size_t)(bs + 1) * (bs + 1) * (bs + 1);
    MeshLds l;
    l.bits_off = (MESH_LDS_VOL + nvox * 4 + 15) & ~(size_t)15;
    l.list_off = (l.bits_off + ((nvox + 63) / 64 + 2) * 8 + 15) & ~(size_t)15;
    l.list_cap = lds_max > l.list_off ? std::min<size_t>((lds_max - l.list_off) / 4, 16384) : 0;
    return l;
}

// k_mesh launch: the register-file variant is the smallest that holds the tape's slots, the
// shape (threads x samples per lane) a per-precision default found by measurement
static int launch_mesh(sdf_tape *t, const void *code, int precision, MeshArgs &a, int grid, int bs, hipStream_t st) {
    sdf_ctx *c = t->ctx;
    const MeshLds l = mesh_lds(bs, c->lds_max);
    if (l.list_off + 4096 > c->lds_max) return fail("sdf_generate: device LDS too small for this batch size");
    a.bits_off = (int)l.bits_off; a.list_off = (int)l.list_off; a.list_cap = (int)l.list_cap;
    const size_t lds = l.list_off + l.list_cap * 4;
    // two slots of sparse tiles share the dense tile's region (deferred emission, k_mesh); a slot has to hold its header,
    // some samples and the cell table of the per-cell counting -- else every tile stays dense
    // -- and between them and the sign bits the area through which a waiting batch's triangles are transposed (the sign bits
    // and the work area stay free: the next work item's record arrives there meanwhile)
    a.slot_bytes = 0; a.stage_off = 0;
    if (c->defer && !a.twopass && a.cull && l.bits_off > MESH_LDS_VOL + 16 * MESH_STAGE_BYTES) {
        const size_t slot = ((l.bits_off - MESH_LDS_VOL - 16 * MESH_STAGE_BYTES) / 2) & ~(size_t)15;
        if (slot >= MESH_SLOT_HDR + 2048 + 8192 && l.list_cap * 4 >= CULL_RECORD) {
            a.slot_bytes = (int)slot;
            a.stage_off = (int)(MESH_LDS_VOL + 2 * slot);
        }
    }
    // the first register-file variant that holds the tape's slots: 0 = (1,1), 1 = (2,2), 2 = (4,2), 3 = (2,4), 4 = (4,4), 5 = (8,8)
    static const uint32_t kFile[6][2] = {{1, 1}, {2, 2}, {4, 2}, {2, 4}, {4, 4}, {8, 8}};
    const uint32_t np = std::max(t->n_p, 1u), nd = std::max(t->n_d, 1u);
    int slots = 5;
    for (int k = 5; k >= 0; k--) if (np <= kFile[k][0] && nd <= kFile[k][1]) slots = k;
    if (c->mesh_slots >= 0 && c->mesh_slots <= 5 && np <= kFile[c->mesh_slots][0] && nd <= kFile[c->mesh_slots][1])
        slots = c->mesh_slots;                                                        // (tuning: another file that fits)
    // (one shape per register file and scheme: 1024 threads x 3 or 2 samples per lane, the 8-slot file 1024 x 1 -- sdf_mesh_inst.hip)
    if (precision != SDF_PRECISION_F64) return fail("k_mesh: float64 only");
    // (a context with a `prof` buffer, SDF_MESH_PROF=1, takes the instrumented instantiations of the same source: the kernels of a normal
    // call hold neither the cycle counters nor the tests for the buffer)
    auto launch = a.prof && c->prof_mesh ? (t->full ? sdf_launch_mesh_f64_full_prof : sdf_launch_mesh_f64_prof)
                                         : (t->full ? sdf_launch_mesh_f64_full : sdf_launch_mesh_f64);
    const int rc = launch(slots, 0, a.twopass, grid, lds, st, (const uint32_t *)code, t->d_c64, a);
    if (rc) return fail(std::string("k_mesh launch: ") + hipGetErrorString((hipError_t)rc));
    return 0;
}

// the per-call statistics from the counters the meshing pass left (end of sdf_generate / sdf_mesh_wait)
static void finish_stats(sdf_tape *t, sdf_mesh *m, const MeshCounters &h, const CallState &s, float ms_prepass, float ms_total) {
    m->work_begin = h.work_begin; m->work_end = h.work_end;
    m->st.n_skipped = s.nb - h.nwork;
    m->st.n_work_begin = m->work_begin; m->st.n_work_end = m->work_end;
    m->st.n_triangles = (int64_t)h.total;
    m->st.n_empty = h.n_empty; m->st.n_nonempty = h.n_nonempty;
    m->st.n_eval_voxels = (int64_t)h.n_eval; m->st.n_ambiguous_cells = (int64_t)h.n_ambiguous;
    m->st.n_pruned_instrs = s.pruning ? (int64_t)h.n_pruned : 0;
    m->st.n_sampled_voxels = (int64_t)h.n_sampled;
    // the kernel's own clock readings: 100 MHz ticks between the first workgroup's start and the last one's end
    m->st.ms_mesh_device = (h.t_first_inv && h.t_last > ~h.t_first_inv) ? (double)(h.t_last - ~h.t_first_inv) * 1e-5 : 0.0;
    m->st.sclk_mhz = h.clk_ticks ? (double)h.clk_cycles / (double)h.clk_ticks * 100.0 : 0.0;
    m->st.t_mesh_first_us = h.t_first_inv ? (double)(~h.t_first_inv) * 0.01 : 0.0;
    m->st.t_mesh_last_us = (double)h.t_last * 0.01;
    m->pruned = s.pruning;
    m->st.mesh_kernel = 1;
    m->st.n_batch_instrs = (int64_t)(s.n_instr - 1) * (h.work_end - h.work_begin);
    t->hint_key = s.key; t->hint_total_tris = std::max<unsigned long long>(h.total, 1);
    {   // (per MODEL and grid, for sdf_generate_records; a handful of entries per job -- the map is emptied when it grows past 4096)
        auto &rh = t->ctx->rec_hints;
        if (rh.size() > 4096) rh.clear();
        sdf_ctx::RecHint &e = rh[std::make_pair(t->content_hash, s.key)];
        e.tris = std::max<unsigned long long>(h.total, 1); e.raw = h.n_raw;
    }
    m->st.ms_prepass = ms_prepass;
    m->st.ms_total = ms_total;
}

// what identifies "the same job on the same grid" for the capacity hints (sdf_tape::hint_key, sdf_ctx::rec_hints)
static unsigned long long grid_key(int nx, int ny, int nz, int bs, int sparse, int64_t shard_index, int64_t shard_count) {
    return ((unsigned long long)nx << 42) ^ ((unsigned long long)ny << 21) ^ (unsigned long long)nz ^
           ((unsigned long long)shard_index << 56) ^ ((unsigned long long)shard_count << 48) ^
           ((unsigned long long)bs << 36) ^ (sparse ? 1ull << 63 : 0ull);
}

// The end of a fused call whose counters have arrived in its slot's pinned staging (the stream was waited for, or the slot's
// `done` event): the counters into h, the event intervals, the look-back time-out.  The statistics are taken unless the
// soup overflowed and the caller repeats the call (stats_if_short: a short SLAB is not repeated here, its call counts as it is).
int finish_call(sdf_mesh *m, const GenCall &call, const CallState &s, bool stats_if_short, MeshCounters &h) {
    sdf_ctx *c = m->ctx;
    CallSlot &cs = c->slots[s.slot];
    h = *(const MeshCounters *)((char *)c->h_stage + (size_t)s.slot * SDF_STAGE_BYTES + SDF_STAGE_BYTES - 256);
    float ms = 0, ms_pre = 0, ms_tot = 0;
    HIPCHK(hipEventElapsedTime(&ms, s.own_start ? cs.e3 : cs.e2, cs.e4));
    HIPCHK(hipEventElapsedTime(&ms_pre, cs.e0, cs.e2));
    HIPCHK(hipEventElapsedTime(&ms_tot, cs.e0, cs.e4));
    m->st.ms_mesh = ms;
    if (h.overflow & 2u) return fail("sdf_generate: ordered-allocation look-back timed out");
    if (!h.overflow || stats_if_short) finish_stats(call.tape, m, h, s, ms_pre, ms_tot);
    return 0;
}

// a free call slot; when all are held by calls in flight, the oldest of them is COLLECTED first (its counters
// and event times live in the slot's pinned staging and events: reusing the slot before sdf_mesh_wait has
// read them would hand that mesh this call's numbers)
static int take_slot(sdf_ctx *c, int &slot) {
    slot = -1;
    for (int k = 0; k < SDF_CALL_SLOTS && slot < 0; k++)
        if (!c->slots[(c->slot_seq + (unsigned)k) % SDF_CALL_SLOTS].busy) slot = (int)((c->slot_seq + (unsigned)k) % SDF_CALL_SLOTS);
    if (slot < 0) {
        slot = (int)(c->slot_seq % SDF_CALL_SLOTS);
        CallSlot &held = c->slots[slot];
        if (held.owner && held.owner->pend.active) { if (sdf_mesh_wait(held.owner, nullptr)) return 1; }
        else { HIPCHK(event_wait(held.done)); }
        held.busy = false; held.owner = nullptr;
    }
    c->slot_seq = (unsigned)slot + 1u;
    return 0;
}

// the host axes into the mesh's device copy (X, then Y, then Z from dX on), through the slot's pinned staging where they fit
static int stage_axes(const GenCall &call, char *stage, double *dX, hipStream_t st) {
    const double *X = call.X, *Y = call.Y, *Z = call.Z;
    const int nx = call.nx, ny = call.ny, nz = call.nz;
    double *dY = dX + nx, *dZ = dY + ny;
    const size_t axis_bytes = (size_t)(nx + ny + nz) * 8;
    if (call.collected && axis_bytes > SDF_STAGE_BYTES - 256) return fail("sdf_generate_to_device_async: axes too long for the staging slot");
    if (axis_bytes <= SDF_STAGE_BYTES - 256) {   // one copy from pinned memory instead of three from pageable
        double *hs = (double *)stage;
        memcpy(hs, X, (size_t)nx * 8); memcpy(hs + nx, Y, (size_t)ny * 8); memcpy(hs + nx + ny, Z, (size_t)nz * 8);
        HIPCHK(hipMemcpyAsync(dX, hs, axis_bytes, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(dX, X, (size_t)nx * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dY, Y, (size_t)ny * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dZ, Z, (size_t)nz * 8, hipMemcpyHostToDevice, st));
    }
    return 0;
}

// capacity of the library's soup for a call's first attempt: from the last call of this tape on the same grid, else
// from the work-list length (one synchronisation: not quiet)
static int first_soup_cap(sdf_tape *t, sdf_mesh *m, unsigned long long key, hipStream_t st, unsigned long long &cap, bool &quiet) {
    if (t->hint_key == key && t->hint_total_tris) {
        cap = t->hint_total_tris + t->hint_total_tris / 4 + 4096;
        return 0;
    }
    MeshCounters h;
    quiet = false;
    HIPCHK(hipMemcpyAsync(&h, m->counters.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
    const unsigned long long nshard0 = (unsigned long long)std::max(h.work_end - h.work_begin, 1);
    cap = std::max<unsigned long long>(4096ull * nshard0, 1ull << 16);
    // a guess, not a need (the overflow re-run finds the exact size): never more than half the free memory
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        cap = std::min<unsigned long long>(cap, std::max<unsigned long long>(free_b / 2 / (72 + 40), 1ull << 16));   // (+ 40 B per triangle: the two-pass arenas)
    return 0;
}

// where an attempt's triangles go: the call's own destination (cap == 0), or a library soup of `cap` triangles
static int soup_target(const GenCall &call, sdf_mesh *m, int attempt, unsigned long long cap, bool &quiet, MeshArgs &a) {
    sdf_ctx *c = m->ctx;
    a.compact = 0; a.xf = nullptr; a.xf_cap = 0; a.raw = nullptr; a.raw_cap = 0;
    if (cap) {
        if (!m->out.p && !c->arena_pool.empty()) { m->out = c->arena_pool.back(); c->arena_pool.pop_back(); }
        if (m->out.bytes < (size_t)cap * 72) quiet = false;     // (an allocation: the stream idles meanwhile)
        if (m->out.ensure((size_t)cap * 72)) {
            // a first-call guess that does not fit: shrink it and let the overflow re-run size the soup exactly
            bool ok = false;
            for (int k = 0; k < 6 && !ok && attempt == 0 && cap > (1ull << 16); k++) {
                cap = std::max<unsigned long long>(cap / 4, 1ull << 16);
                ok = m->out.ensure((size_t)cap * 72) == 0;
            }
            if (!ok) return 1;
        }
        a.out = (double *)m->out.p; a.out_cap = m->out.bytes / 72;
    } else if (call.dest == GenCall::SLAB) {
        unsigned char *d_slab = (unsigned char *)call.d_out;
        const SlabLayout L(call.cap_items, call.cap_tris);
        a.out = reinterpret_cast<double *>(d_slab + L.tris_off); a.out_cap = (unsigned long long)call.cap_tris;
        a.compact = 1; a.xf = reinterpret_cast<double *>(d_slab + L.xf_off);
        a.raw = reinterpret_cast<float *>(d_slab + L.raw_off); a.raw_cap = L.raw_cap;
        a.xf_cap = (int)std::min<int64_t>(call.cap_items, 0x7fffffff);
    } else {
        a.out = (double *)call.d_out; a.out_cap = (unsigned long long)call.cap_tris;
    }
    return 0;
}

// One meshing attempt on `st`, up to the counters' copy into the slot's pinned staging: k_mesh [-> k_scan_items -> k_emit2]
// [-> k_pack_slab].  soup_cap: see soup_target; quiet: nothing but k_mesh follows ev[2] on the stream, and the host did not
// stall in between; tail: work items at the list's end that k_mesh hands out by k_cull's cost estimates (0: in order).
static int mesh_attempt(const GenCall &call, sdf_mesh *m, CallState &s, hipStream_t st, int attempt, unsigned long long soup_cap, bool quiet,
                        bool culling, int tail, int tape_stride) {
    sdf_tape *t = call.tape;
    sdf_ctx *c = t->ctx;
    CallSlot &cs = c->slots[s.slot];
    const int nb = s.nb;
    const uint32_t n_instr = s.n_instr;
    MeshArgs a;
    a.twopass = 0; a.desc = nullptr; a.cells = nullptr; a.tlist = nullptr; a.cells_cap = a.tlist_cap = 0; a.block_item = nullptr;
    a.order = tail ? (const int *)m->order.p : nullptr; a.tail = tail;
    if (soup_target(call, m, attempt, soup_cap, quiet, a)) return 1;
    if (attempt) {   // (the first pass finds both cleared by k_compact)
        HIPCHK(hipMemsetAsync(m->counters.p, 0, MESH_COUNTERS_RESET_BYTES, st));
        HIPCHK(hipMemsetAsync(m->status.p, 0, (size_t)nb * 8, st));
    }
    a.g = m->g; a.worklist = (const int *)m->worklist.p;
    a.kinds = (unsigned char *)m->kinds.p; a.status = (unsigned long long *)m->status.p;
    a.ctr = (MeshCounters *)m->counters.p;
    a.mc = (const McTables *)c->mc.p;
    a.prof = (unsigned long long *)c->prof.p;
    // One pass or two?  (decided here: the two-pass scheme parks nothing -- its triangles are numbered by k_scan_items -- so a
    // call that takes it does not make its lane allocate park slots: 1.2 GB that the long jobs' lanes never touched, r04 advisor)
    const bool twopass = c->twopass >= 0 ? c->twopass != 0 : n_instr > 96;
    DevBuf &park = call.collected ? cs.park : c->park;   // (k_mesh kernels of calls in flight may overlap in time, whichever
                                                         // streams they run on: each call slot has its own staging slots)
    const bool parks = c->parking && !twopass;
    if (parks && !park.p) { quiet = false; if (park.ensure((size_t)c->n_cu * MESH_PARK_DEPTH * SDF_PARK_TRIS * 36)) return 1; }
    a.park = parks ? (float *)park.p : nullptr; a.park_cap = a.park ? SDF_PARK_TRIS : 0;
    a.park_spins = (unsigned)c->park_spins;
    a.cull = culling ? (const unsigned char *)m->cull.p : nullptr;
    a.tape_stride = tape_stride;
    a.n_instr = (int)n_instr;
    // One pass or two?  The one-pass kernel (look-back + parking inside the sampling kernel) is 7 - 20 % faster on
    // short tapes: it hides its triangle traffic behind other workgroups' arithmetic, which three kernels in a row
    // cannot.  On long tapes (weave at 2^33, 244 instructions) the two schemes tie -- 27.5 vs 28.0 ms -- and the
    // two-pass one moves a third of the bytes (9 GB against 25 GB per call: no parking, and the 4-slot sampling
    // kernel spills less without the emit phases): the tape's length decides (sdf_ctx_set_twopass / SDF_MESH_TWOPASS
    // override).
    if (twopass) {
        // the arenas of the two-pass scheme: a surface cell carries at least one triangle, so the soup's capacity
        // bounds both (a call whose arenas turn out too small is flagged and repeated like one whose soup is)
        const size_t cap_t = (size_t)a.out_cap;
        if (m->desc.bytes < (size_t)nb * sizeof(ItemDesc) || m->cellrecs.bytes < cap_t * 36 || m->trilist.bytes < cap_t * 4) quiet = false;
        if (m->desc.ensure((size_t)nb * sizeof(ItemDesc)) || m->cellrecs.ensure(cap_t * 36) || m->trilist.ensure(cap_t * 4) ||
            m->blockidx.ensure(((cap_t + 255) / 256 + 2) * sizeof(int)))
            return 1;
        a.twopass = 1; a.desc = (ItemDesc *)m->desc.p; a.cells = (unsigned *)m->cellrecs.p; a.tlist = (unsigned *)m->trilist.p;
        a.block_item = (const int *)m->blockidx.p;
        a.cells_cap = a.tlist_cap = (unsigned long long)cap_t;
    }
    if (a.prof) {   // (words 16.. are k_cull's: cleared before the prepass; behind byte 512: the workgroups' timelines)
        HIPCHK(hipMemsetAsync(a.prof, 0, 128, st));
        HIPCHK(hipMemsetAsync((unsigned char *)a.prof + 512, 0, 4096 * 32, st));
    }
    const int grid = std::min(nb, c->n_cu);   // persistent workgroups; surplus ones find the list empty
    s.own_start = attempt > 0 || a.prof || !quiet;   // (something was enqueued, or the host waited, since ev[2])
    if (s.own_start) HIPCHK(hipEventRecord(cs.e3, st));
    if (launch_mesh(t, tape_stride ? m->tapes.p : (const void *)t->d_code, call.precision, a, grid, call.bs, st)) return 1;
    if (a.twopass) {
        const unsigned long long emit_blocks = (a.out_cap + 255ull) / 256ull;
        if (emit_blocks > 0x7fffffffull) return fail("sdf_generate: soup capacity too large for one k_emit2 launch");
        launch_k_scan_items(dim3(1), dim3(1024), st, (const ItemDesc *)m->desc.p, (MeshCounters *)m->counters.p,
                           (unsigned long long *)m->status.p, (int *)m->blockidx.p, emit_blocks + 1ull);
        launch_k_emit2(dim3((unsigned)std::max<unsigned long long>(emit_blocks, 1ull)), dim3(256), st, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(cs.e4, st));
    if (call.dest == GenCall::SLAB) {
        const unsigned pack_blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((call.cap_items + 255) / 256, 1), 1024);
        HIPCHK((hipError_t)sdf_launch_pack_slab(pack_blocks, st, (const MeshCounters *)m->counters.p, (const unsigned long long *)m->status.p,
                                                (unsigned char *)call.d_out, (long long)call.cap_items, (long long)call.cap_tris));
    }
    MeshCounters *hp = (MeshCounters *)((char *)c->h_stage + (size_t)s.slot * SDF_STAGE_BYTES + SDF_STAGE_BYTES - 256);   // pinned
    HIPCHK(hipMemcpyAsync(hp, m->counters.p, sizeof(MeshCounters), hipMemcpyDeviceToHost, st));
    return 0;
}

// SDF_MESH_PROF=1: what k_cull and the `grid` workgroups of k_mesh counted during the call that has just completed, to stderr
static int mesh_prof_report(sdf_ctx *c, int grid, float ms) {
    unsigned long long pc[64];
    HIPCHK(hipMemcpy(pc, c->prof.p, 512, hipMemcpyDeviceToHost));
    {   // timeline of the workgroups: when each ran out of work and when it was done, relative to the first start
        std::vector<unsigned long long> tl((size_t)4 * grid);
        HIPCHK(hipMemcpy(tl.data(), (unsigned char *)c->prof.p + 512, tl.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t_end = 0;
        double s_out = 0, s_done = 0, mn_out = 1e30, mx_out = 0;
        for (int i = 0; i < grid; i++) t0 = std::min(t0, tl[4 * i]);
        for (int i = 0; i < grid; i++) {
            const double o = (double)(tl[4 * i + 1] - t0) * 0.01, d = (double)(tl[4 * i + 2] - t0) * 0.01;   // us
            s_out += o; s_done += d; mn_out = std::min(mn_out, o); mx_out = std::max(mx_out, o); t_end = std::max(t_end, tl[4 * i + 2]);
        }
        double first_hi = 0;   // the latest start: workgroups that were not resident from the beginning start late
        for (int i = 0; i < grid; i++) first_hi = std::max(first_hi, (double)(tl[4 * i] - t0) * 0.01);
        fprintf(stderr, "[k_mesh prof] %d workgroups (1 per CU), last of them started after %.1f us; out of work after min %.1f avg %.1f max %.1f us; done after avg %.1f, last %.1f us\n",
                grid, first_hi, mn_out, s_out / grid, mx_out, s_done / grid, (double)(t_end - t0) * 0.01);
    }
    fprintf(stderr, "[k_cull prof] work items by listed tasks (of 563; bins of 64, last: not culled): %llu %llu %llu %llu %llu %llu %llu %llu %llu | %llu\n",
            pc[32], pc[33], pc[34], pc[35], pc[36], pc[37], pc[38], pc[39], pc[40], pc[41]);
    fprintf(stderr, "[k_cull prof] cycles of thread 0, summed over the workgroups: start %llu boxes %llu list %llu groups %llu (%llu passes, %llu groups) tasks %llu record %llu\n",
            pc[16], pc[17], pc[18], pc[19], pc[23], pc[22], pc[20], pc[21]);
    fprintf(stderr, "[k_cull prof] task listing: which tasks %llu, scans %llu; start: range %llu batch %llu origin %llu axes %llu barrier %llu (rest: tape length)\n", pc[24], pc[25], pc[26], pc[27], pc[30], pc[28], pc[29]);
    fprintf(stderr, "[k_mesh prof] sampling: intervals %llu task list %llu interpreter %llu sign bits %llu\n", pc[8], pc[9], pc[10], pc[11]);
    fprintf(stderr, "[k_mesh prof] fine: atomic %llu barrier+rank %llu header %llu | rows %llu cells %llu | placing %llu look-back %llu | round end %llu\n",
            pc[42], pc[43], pc[44], pc[45], pc[46], pc[47], pc[48], pc[49]);
    fprintf(stderr, "[k_mesh prof] %.3f ms; cycles/WG-sum: grab %llu sample %llu count %llu (of which placing the parked batch %llu) list %llu emit %llu tail %llu; %llu batches parked, %llu written one batch later from their slot\n",
            ms, pc[0], pc[1], pc[2], pc[6], pc[3], pc[4], pc[5], pc[7], pc[12]);
    return 0;
}

int generate_impl(sdf_mesh *m, const GenCall &call) {
    sdf_tape *t = call.tape;
    sdf_ctx *c = t->ctx;
    const bool slab = call.dest == GenCall::SLAB;
    const int nx = call.nx, ny = call.ny, nz = call.nz;
    CallState s;
    if (take_slot(c, s.slot)) return 1;
    CallSlot &cs = c->slots[s.slot];
    // Calls in flight (sdf_generate_to_device_async) each run on their slot's OWN stream: call i + 1's prepass then
    // fills the compute units that call i's k_mesh leaves idle in its tail (a persistent workgroup per CU, the last
    // batches finish at different times: 9 % of that kernel's CU-time) and the dispatch gaps of one call hide behind
    // the kernels of the other.  Everything a call touches is its own (per-mesh buffers, per-slot staging / events /
    // park slots), so the streams need no ordering among themselves.  An adopted caller stream is never left.
    const bool own_lane = call.collected && !slab && c->stream == c->own_stream && c->slot_streams;
    hipStream_t st = call.lane ? call.lane : (own_lane ? cs.stream : c->stream);
    m->stream = (own_lane || call.lane) ? st : nullptr;
    if (grid_batches(nx, ny, nz, call.bs, "sdf_generate", m->g, s.nb)) return 1;
    const int nb = s.nb;
    m->st.n_batches = nb;
    m->st.n_grid_voxels = (int64_t)nx * ny * nz;
    if (nb == 0) {
        if (slab) HIPCHK(hipMemsetAsync(call.d_out, 0, sizeof(SlabHeader), st));   // an empty grid: an empty slab
        return 0;
    }

    if (m->axes.ensure((size_t)(nx + ny + nz) * 8) || m->kinds.ensure((size_t)nb) || m->worklist.ensure((size_t)nb * 4) ||
        m->status.ensure((size_t)nb * 8))
        return 1;
    if (!m->counters.p && !c->counter_pool.empty()) { m->counters = c->counter_pool.back(); c->counter_pool.pop_back(); }
    if (m->counters.ensure(sizeof(MeshCounters))) return 1;
    double *dX = (double *)m->axes.p;
    m->g.X = dX; m->g.Y = dX + nx; m->g.Z = dX + nx + ny;
    HIPCHK(hipEventRecord(cs.e0, st));
    if (stage_axes(call, (char *)c->h_stage + (size_t)s.slot * SDF_STAGE_BYTES, dX, st)) return 1;

    // (three event records per call, not one per interval: each is a marker packet the queue has to drain to;
    // ms_prepass = ev[0] -> ev[2] includes the copy of the axes, ms_mesh = ev[2] -> ev[4], ms_total = ev[0] -> ev[4])
    // interval pass: per batch, which instructions never matter (float64 sampling only: the intervals
    // bound the float64 interpreter, not the float32 one).  The box of a batch is spanned by its first
    // and last coordinate per axis: monotone axes only.
    auto monotone = [](const double *a, int n) {
        bool up = true, down = true;
        for (int i = 1; i < n; i++) { up &= a[i - 1] <= a[i]; down &= a[i - 1] >= a[i]; }
        return up || down;
    };
    s.n_instr = t->n_words / 2;
    // (t->ia_off: a tape whose constants make the model NaN -- the interval forms keep no NaN through a later clip or min / max)
    const bool intervals_ok = call.precision == SDF_PRECISION_F64 && !t->ia_off && monotone(call.X, nx) && monotone(call.Y, ny) && monotone(call.Z, nz);
    s.pruning = c->prune && t->d_rstart && s.n_instr <= 256 && intervals_ok && t->n_consts < 0xFFFFF0u;
    // 64-bit words per batch tape: the instructions, one more END, the length; whole 64-byte lines
    const int tape_stride = s.pruning ? (int)((s.n_instr + 2 + 7) & ~7u) : 0;
    if (enqueue_prepass(call, m, nb, tape_stride, st)) return 1;
    // (k_mesh reads the batch's cull record into the list region of its LDS, which has to hold it)
    const bool culling = c->cull && intervals_ok && t->ia_complete && mesh_lds(call.bs, c->lds_max).list_off + CULL_RECORD <= c->lds_max;
    // the tail of the work list is handed out by descending cost (MeshArgs::order, k_cull's estimates); fewer items
    // than k_mesh has workgroups
    const int tail_max = std::min<int>(MESH_TAIL_MAX, std::min(nb, c->n_cu) - 1);
    // (not for calls in flight next to others: the argument that a reordered tail cannot stall -- fewer tail items than
    // workgroups -- counts RESIDENT workgroups, and a k_mesh that shares the device with another call's k_mesh may have
    // fewer of them for a while; the neighbours fill the tail of such a call anyway)
    const bool tail_order = culling && c->tail_order && tail_max >= 2 && !call.collected;
    s.key = grid_key(nx, ny, nz, call.bs, call.sparse, call.shard_index, call.shard_count);
    if (culling && enqueue_cull(t, m, nb, tape_stride, tail_order, tail_max, st)) return 1;
    HIPCHK(hipEventRecord(cs.e2, st));

    // ---- meshing.  The whole chain (prepass -> k_mesh) is enqueued without a host round trip: the
    // work-list length stays on the device and k_mesh writes the ordered float64 soup itself.  The
    // soup goes into the caller's device buffer when one was given (sdf_generate_to_device),
    // otherwise into a library buffer sized from the last call of this tape on the same grid (first
    // call: from the work-list length, which costs one synchronisation).  A soup that does not fit
    // is detected on the device (nothing is written past the capacity) and the pass is re-run into
    // a library buffer of the exact size. ----
    unsigned long long soup_cap = 0;   // (0: into the call's own destination)
    bool quiet = true;     // nothing but k_mesh follows ev[2] on the stream, and the host did not stall in between
    if (call.dest == GenCall::SOUP && first_soup_cap(t, m, s.key, st, soup_cap, quiet)) return 1;
    for (int attempt = 0;; attempt++) {
        if (mesh_attempt(call, m, s, st, attempt, soup_cap, quiet, culling, tail_order ? tail_max : 0, tape_stride)) return 1;
        if (call.collected) {   // the caller collects the result with sdf_mesh_wait
            HIPCHK(hipEventRecord(cs.done, st));
            cs.busy = true; cs.owner = m;
            sdf_mesh::Pending &pd = m->pend;
            pd.active = true; pd.call = call; pd.got = s;
            pd.axes.assign(call.X, call.X + nx); pd.axes.insert(pd.axes.end(), call.Y, call.Y + ny); pd.axes.insert(pd.axes.end(), call.Z, call.Z + nz);
            pd.call.X = pd.axes.data(); pd.call.Y = pd.call.X + nx; pd.call.Z = pd.call.Y + ny;
            return 0;
        }
        HIPCHK(stream_wait(st));
        MeshCounters h;
        const int rc = finish_call(m, call, s, slab, h);
        if (c->prof.p && mesh_prof_report(c, std::min(nb, c->n_cu), m->st.ms_mesh)) return 1;
        m->st.n_retries = attempt;
        if (rc) return 1;
        if (slab) {   // (the synchronous records mode, sdf_generate_records: its caller sizes the slab again and repeats the call)
            const SlabLayout L(call.cap_items, call.cap_tris);
            const bool raw_over = (long long)h.n_raw > L.raw_cap;
            m->n_raw = (long long)h.n_raw;
            m->rec_overflow = (h.overflow & 1u) != 0 || raw_over || (long long)(h.work_end - h.work_begin) > (long long)call.cap_items;
            m->rec_need_tris = std::max<long long>((long long)h.total, raw_over ? (long long)h.n_raw * SLAB_RAW_DIV : 0ll);
            m->emitted_to = nullptr;
            return 0;
        }
        if (!h.overflow) {
            m->emitted_to = soup_cap ? nullptr : call.d_out;
            return 0;
        }
        if (attempt >= 3) return fail("sdf_generate: soup buffer overflow persists");
        soup_cap = h.total + 1024;               // the exact need is known now: h.total
    }
}

extern "C" {

// every check and message of sdf_generate, then the call: fused, or through device memory for batch_size > 32
static int generate_entry(const GenCall &call, sdf_mesh **out) {
    sdf_tape *t = call.tape;
    const int bs = call.bs, precision = call.precision;
    if (!t || !call.X || !call.Y || !call.Z || !out) return fail("sdf_generate: NULL argument");
    *out = nullptr;
    if (t->n_extern) return fail("sdf_generate: the tape reads user closures (L_EXTERN): mesh it with sdf_generate_field");
    if (bs < 1 || bs > SDF_BATCH_SIZE_MAX) return fail("sdf_generate: batch_size must be in 1..512");
    if (bs > 32 && call.dest == GenCall::SLAB) return fail("sdf_generate_compact: batch_size must be in 1..32 (batches of more than 33^3 samples are not part of the multi-GPU exchange)");
    if (bs > 32 && call.d_kinds) return fail("sdf_generate_from_kinds: batch_size must be in 1..32");
    if (call.shard_count < 1 || call.shard_index < 0 || call.shard_index >= call.shard_count) return fail("sdf_generate: bad shard");
    if (precision == SDF_PRECISION_F32)
        return fail("sdf_generate: the meshing path samples in float64 (the reference's arithmetic); SDF_PRECISION_F32 was a diagnostic until round 4 -- "
                    "outside the 1e-5 tolerance at its maximum, slower than float64 behind the interval passes -- and was removed; sdf_eval_* and "
                    "sdf_estimate_bounds keep both precisions");
    if (precision != SDF_PRECISION_F64) return fail("sdf_generate: bad precision");
    if (call.nx < 0 || call.ny < 0 || call.nz < 0) return fail("sdf_generate: negative axis length");
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    sdf_mesh *m = new sdf_mesh();
    m->ctx = c;
    // (batch_size > 32: through device memory, synchronously, into library memory -- a caller buffer is reported as not filled,
    // like one that was too small: sdf_mesh_emit_device copies)
    if (bs > 32 ? generate_big(m, call) : generate_impl(m, call)) {
        const std::string keep = g_err;
        sdf_mesh_destroy(m);
        g_err = keep;
        return 1;
    }
    *out = m;
    return 0;
}

int sdf_generate(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs,
                 int sparse, int64_t shard_index, int64_t shard_count, int precision, sdf_mesh **out) {
    return generate_entry(gen_call(t, X, nx, Y, ny, Z, nz, bs, sparse, shard_index, shard_count, precision), out);
}

int sdf_generate_to_device(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs,
                           int sparse, int64_t shard_index, int64_t shard_count, int precision, void *d_out,
                           int64_t cap_tris, int *emitted, sdf_mesh **out) {
    if (emitted) *emitted = 0;
    if (!d_out || cap_tris <= 0) return fail("sdf_generate_to_device: output buffer is NULL or empty");
    GenCall call = gen_call(t, X, nx, Y, ny, Z, nz, bs, sparse, shard_index, shard_count, precision);
    call.dest = GenCall::CALLER; call.d_out = d_out; call.cap_tris = cap_tris;
    if (generate_entry(call, out)) return 1;
    if (emitted) *emitted = ((*out)->emitted_to == d_out || (*out)->st.n_triangles == 0) ? 1 : 0;
    return 0;
}

int sdf_generate_from_kinds(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs,
                            int64_t shard_index, int64_t shard_count, int precision, const void *d_kinds, sdf_mesh **out) {
    if (!d_kinds) return fail("sdf_generate_from_kinds: d_kinds is NULL");
    GenCall call = gen_call(t, X, nx, Y, ny, Z, nz, bs, 1, shard_index, shard_count, precision);
    call.d_kinds = (const unsigned char *)d_kinds;
    return generate_entry(call, out);
}

int sdf_generate_to_device_async(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs,
                                 int sparse, int64_t shard_index, int64_t shard_count, int precision, void *d_out,
                                 int64_t cap_tris, sdf_mesh **out) {
    if (!d_out || cap_tris <= 0) return fail("sdf_generate_to_device_async: output buffer is NULL or empty");
    GenCall call = gen_call(t, X, nx, Y, ny, Z, nz, bs, sparse, shard_index, shard_count, precision);
    call.dest = GenCall::CALLER; call.d_out = d_out; call.cap_tris = cap_tris;
    call.collected = true;
    return generate_entry(call, out);
}

// `generate` for a caller who wants the soup ON THE HOST (what the reference's `generate` returns, sdf/core.py:131-141): the triangles
// are written as 16-byte records into a slab of the library's (sdf_slab.h: local float32 coordinates + a transform per work item,
// the multi-GPU exchange unit) instead of as 72-byte float64 triangles, and sdf_mesh_emit_host_workers makes the float64 soup on host
// threads while the records are still arriving: 47 MB over PCIe instead of 212 MB at 512^3.  The slab is sized from what the last
// call of the same MODEL on the same grid needed (sdf_ctx::rec_hints, keyed by the tape's content: a fresh tape object of the same
// model finds it); without such a hint -- the first call -- the call is an ordinary sdf_generate, which leaves the hint.  A slab that
// turns out too small is sized again and the call repeated.  The mesh answers every reader: those that want the float64 soup on
// the device (STL records, weld, sdf_mesh_emit_device, ranges) get it from k_expand on demand.
int sdf_generate_records(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs,
                         int sparse, int precision, sdf_mesh **out) {
    if (!t || !X || !Y || !Z || !out) return fail("sdf_generate_records: NULL argument");
    sdf_ctx *c = t->ctx;
    const unsigned long long key = grid_key(nx, ny, nz, bs, sparse, 0, 1);
    const auto it = c->rec_hints.find(std::make_pair(t->content_hash, key));
    GridDesc g;
    const long long nb64 = grid_desc(nx, ny, nz, bs, g);
    GenCall call = gen_call(t, X, nx, Y, ny, Z, nz, bs, sparse, 0, 1, precision);
    if (bs < 1 || bs > 32 || t->n_extern || it == c->rec_hints.end() || nb64 <= 0 || nb64 > 0x7fffffffLL || precision != SDF_PRECISION_F64)
        return generate_entry(call, out);     // (every check and message of sdf_generate)
    HIPCHK(set_device(c->device));
    long long cap_tris = (long long)(it->second.tris + it->second.tris / 64 + 1024);
    if ((long long)it->second.raw > cap_tris / SLAB_RAW_DIV + SLAB_RAW_MIN) cap_tris = std::max<long long>(cap_tris, (long long)(it->second.raw + it->second.raw / 8) * SLAB_RAW_DIV);
    *out = nullptr;
    sdf_mesh *m = new sdf_mesh();
    m->ctx = c;
    m->records = true;
    int attempt = 0;
    for (;; attempt++) {
        m->slab_items = nb64; m->slab_tris = cap_tris;
        const SlabLayout L(m->slab_items, m->slab_tris);
        int rc = m->slab.ensure(L.bytes);
        call.dest = GenCall::SLAB; call.d_out = m->slab.p; call.cap_items = m->slab_items; call.cap_tris = cap_tris;
        if (!rc) rc = generate_impl(m, call);
        if (!rc && m->rec_overflow && attempt >= 3) rc = fail("sdf_generate_records: slab overflow persists");
        if (rc) {
            const std::string keep = g_err;
            sdf_mesh_destroy(m);
            g_err = keep;
            return 1;
        }
        if (!m->rec_overflow) break;
        cap_tris = m->rec_need_tris + m->rec_need_tris / 64 + 1024;
    }
    m->st.n_retries = attempt;
    *out = m;
    return 0;
}

size_t sdf_slab_bytes(int64_t cap_items, int64_t cap_tris) {
    if (cap_items < 0 || cap_tris < 0) return 0;
    return SlabLayout(cap_items, cap_tris).bytes;
}

int sdf_generate_compact_async(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs,
                               int sparse, int64_t shard_index, int64_t shard_count, int precision, void *d_slab,
                               int64_t cap_items, int64_t cap_tris, sdf_mesh **out) {
    if (!d_slab || cap_items < 0 || cap_tris < 0) return fail("sdf_generate_compact_async: slab is NULL or its capacities are negative");
    GenCall call = gen_call(t, X, nx, Y, ny, Z, nz, bs, sparse, shard_index, shard_count, precision);
    call.dest = GenCall::SLAB; call.d_out = d_slab; call.cap_items = cap_items; call.cap_tris = cap_tris;
    call.collected = true;
    return generate_entry(call, out);
}

int sdf_expand_slabs(sdf_ctx *c, const void *const *d_slabs, int n_slabs, int64_t cap_items, int64_t cap_tris, void *d_out, int64_t cap_out) {
    if (!c || !d_slabs || (!d_out && cap_out > 0)) return fail("sdf_expand_slabs: NULL argument");
    if (n_slabs < 1 || n_slabs > 64) return fail("sdf_expand_slabs: 1..64 slabs");
    if (cap_items < 0 || cap_tris < 0 || cap_out < 0) return fail("sdf_expand_slabs: negative capacity");
    if (cap_items == 0 || cap_out == 0) return 0;
    HIPCHK(set_device(c->device));
    SlabPtrs ptrs = {};
    for (int i = 0; i < n_slabs; i++) { if (!d_slabs[i]) return fail("sdf_expand_slabs: NULL slab"); ptrs.p[i] = (const unsigned char *)d_slabs[i]; }
    const unsigned long long blocks = ((unsigned long long)cap_out + 255ull) / 256ull;
    if (blocks > 0x7fffffffull) return fail("sdf_expand_slabs: soup capacity too large for one launch");
    HIPCHK((hipError_t)sdf_launch_expand(c->stream, ptrs, n_slabs, (long long)cap_items, (long long)cap_tris, (double *)d_out, (unsigned long long)cap_out));
    return 0;
}

}  // extern "C"
