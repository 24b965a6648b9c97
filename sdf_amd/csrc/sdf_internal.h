// sdf_internal.h -- what the handles of the C ABI (include/sdf_hip.h) point to: the context, a tape, a mesh, and the descriptor of a
// generate call; plus the few functions of the generate pipeline (sdf_generate.hip), of the kernels it launches (sdf_prepass.hip,
// sdf_eval.hip), of its paths through device memory (sdf_chunked.hip) and of the mesh readers (sdf_mesh_out.hip) that another translation unit calls.  With sdf_runtime.h, all a unit needs to define an extern "C" entry point that takes a handle.
#pragma once
#include <cstdint>
#include <map>

#include "../../include/sdf_hip.h"
#include "sdf_chunk_plan.h"   // (SDF_BATCH_SIZE_MAX)
#include "sdf_device.h"
#include "sdf_runtime.h"

using sdfk::DevBuf;
using sdfk::GridDesc;

#define SDF_STAGE_BYTES (1u << 20)
// Calls in flight on one context (sdf_generate_to_device_async): each owns a slot = its pinned staging
// (axes on the way in, counters on the way out) and its events; a slot is reused only after the call that
// held it has completed.
// (eight since r04: with six calls in flight the 512^3 example steps in 0.237 ms, with four in 0.248, same box alternating;
// a lane's park slots -- 1.2 GB -- are allocated when the lane is first used)
#ifndef SDF_CALL_SLOTS
#define SDF_CALL_SLOTS 8
#endif
struct CallSlot {
    hipEvent_t e0 = nullptr, e2 = nullptr, e3 = nullptr, e4 = nullptr;   // start, prepass end, k_mesh start (re-runs), k_mesh end
    hipEvent_t done = nullptr;                                            // behind the counters' copy to the host
    bool busy = false;
    struct sdf_mesh *owner = nullptr;                                     // the in-flight mesh whose counters / events the slot holds
    hipStream_t stream = nullptr;                                         // the lane asynchronous calls of this slot run on
    DevBuf park;                                                          // ... and its k_mesh staging slots
};
#define SDF_PARK_TRIS 8192   // triangles per workgroup staging slot of k_mesh (36 bytes each); larger batches wait instead
                             // (16 slots per workgroup: 1.2 GB per call lane, allocated on a lane's first use; with 4096
                             // per slot weave at 2^33 has batches that cannot park: 30.3 instead of 27.7 ms)

struct sdf_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev[8] = {};
    int n_cu = 256;
    size_t lds_max = 0;
    DevBuf scratch_in, scratch_out, rows, rows_off, mc;
    DevBuf ext;                       // closure points / values of sdf_eval_*extern* (L_EXTERN leaves)
    DevBuf field_vals, field_vol, field_tiles;   // sdf_chunked.hip: a chunk's sampled values (f64, sdf_generate_field), volumes (f32), tile table
    DevBuf prof;                      // SDF_MESH_PROF=1: per-phase cycle counters of k_mesh (diagnostics)
    int prof_mesh = 1;                // ... counted by the INSTRUMENTED instantiations of k_mesh (sdf_mesh_inst.hip, -DMESH_PROF=1), which a context with the
                                      // buffer launches.  SDF_MESH_PROF=2: the buffer and the report, but the plain kernels (their words must stay zero: a test)
    int prune = 1;                    // SDF_PRUNE=0 switches the interval prepass off (diagnostics)
    int parking = 1;                  // SDF_PARK=0: k_mesh waits for its predecessors instead of parking a batch (diagnostics)
    int cull = 1;                     // SDF_CULL=0: k_mesh samples every voxel of a batch instead of deciding cell groups by intervals
    int prune_list_min = 8192;        // SDF_PRUNE_LIST_MIN: from this many batches on the interval prepass runs behind k_compact, over the work list
    int park_spins = 1;               // SDF_PARK_SPINS: polls before parking (tuning; measured: waiting never pays)
    DevBuf park;                      // k_mesh's staging slots, one per CU (allocated by the first sdf_generate)
    int mesh_slots = -1;              // SDF_MESH_SLOTS override of the register-file variant (tuning)
    std::vector<DevBuf> arena_pool;   // soup buffers handed back by destroyed meshes
    std::vector<DevBuf> counter_pool; // 64-byte MeshCounters blocks handed back by destroyed meshes
    void *h_stage = nullptr;          // pinned host staging, SDF_CALL_SLOTS x SDF_STAGE_BYTES
    CallSlot slots[SDF_CALL_SLOTS];
    unsigned slot_seq = 0;
    int slot_streams = 1;             // SDF_SLOT_STREAMS=0: asynchronous calls stay on the context's stream (diagnostics)
    int cull_block = 0;               // SDF_CULL_BLOCK=64 / 128 / 256: threads per work item of k_cull (0: the default of the variant)
    int tail_order = 1;               // SDF_TAIL_ORDER=0: k_mesh takes the whole work list in order
    int twopass = -1;                 // SDF_MESH_TWOPASS=0 / 1: force the one-pass k_mesh (look-back + parking) resp. k_mesh / k_scan_items / k_emit2
    int defer = 1;                    // SDF_DEFER=0: k_mesh keeps every tile dense and writes (or parks) a batch's triangles right after counting it
    int cull_levels = 0;              // SDF_CULL_LEVELS=2 / 3: interval levels of k_cull (3: + sub-groups of 2^3 cells); 0: by the tape (see enqueue_cull)
    DevBuf bounds_work;               // k_estimate_bounds_w: the waves' exchange words (tagged per call, sdf_bounds.hip)
    unsigned bounds_tag = 0, bounds_tag0 = 0;
    // sdf_generate_records: what the last call of a MODEL (content hash) on a grid needed -- triangles, raw-area triangles -- so that the
    // next one, possibly through a fresh tape object of the same model, can size its slab without a host round trip
    struct RecHint { unsigned long long tris = 0, raw = 0; };
    std::map<std::pair<unsigned long long, unsigned long long>, RecHint> rec_hints;
    void *h_rec = nullptr;            // pinned staging of sdf_mesh_emit_host_workers: a slab's head, raw area and records on their way to the host threads
    size_t h_rec_bytes = 0;
    std::vector<hipEvent_t> rec_ev;   // ... one event per piece of the copy
};

struct sdf_tape {
    sdf_ctx *ctx = nullptr;
    uint32_t *d_code = nullptr;
    double *d_c64 = nullptr;
    float *d_c32 = nullptr;
    uint32_t n_words = 0, n_consts = 0;
    bool full = false;
    uint32_t n_p = 0, n_d = 0;
    uint16_t *d_rstart = nullptr, *d_lstart = nullptr;   // operand ranges of the prunable combines (or NULL)
    bool ia_complete = false;                            // every op has an interval form (sdf_interval.h ia_has_form)
    bool ia_rare = false;                                // ... one of them a leaf of ia_leaf_rare (the k_cull variant that knows them)
    bool ia_off = false;                                 // the lowering found that the model can be NaN everywhere: no interval pass (sdf_tape_set_intervals)
    uint32_t n_extern = 0;                               // user closures the tape reads through L_EXTERN leaves (sdf_eval_points_extern_*)
    unsigned long long hint_key = 0, hint_total_tris = 0;   // arena sizing: last call of this tape
    unsigned long long content_hash = 0;                    // FNV-1a of the code words and the constants' bits: what identifies the MODEL,
                                                            // on every rank alike and whatever address the tape object lands on (sdf_comm.hip)
};

// What one fused call (prepass -> k_cull -> k_mesh) is asked to do.  The entry points build one by naming fields; a call in
// flight keeps its descriptor in sdf_mesh::Pending.
struct GenCall {
    sdf_tape *tape = nullptr;
    const double *X = nullptr, *Y = nullptr, *Z = nullptr;   // the host's axes
    int nx = 0, ny = 0, nz = 0, bs = 0, sparse = 0, precision = 0;
    int64_t shard_index = 0, shard_count = 1;
    // where the triangles go.  SOUP: a library buffer sized from the last call of the tape on the grid; CALLER: d_out, cap_tris
    // float64 triangles; SLAB: compact mode (sdf_generate_compact_async, sdf_generate_records) -- d_out is a SLAB of capacity
    // (cap_items, cap_tris)
    enum Dest { SOUP, CALLER, SLAB } dest = SOUP;
    void *d_out = nullptr;
    int64_t cap_tris = 0, cap_items = 0;
    bool collected = false;                   // the call returns in flight and sdf_mesh_wait finishes it (else: synchronous)
    hipStream_t lane = nullptr;               // the stream the whole call is enqueued on (the exchange steps of sdf_comm run on lanes of their own)
    // the skip test's verdict for every batch is already on the device (0 skipped / 255 pending, n_batches
    // bytes: sdf_skip_kinds, possibly all-gathered from the ranks that each tested a share): k_skip is not run
    const unsigned char *d_kinds = nullptr;
};
// ... and what the call learned while it was enqueued: finishing it needs these
struct CallState { int slot = 0, nb = 0; bool pruning = false, own_start = false; uint32_t n_instr = 0; unsigned long long key = 0; };

struct sdf_mesh {
    sdf_ctx *ctx = nullptr;
    sdf_stats st = {};
    GridDesc g = {};
    DevBuf axes, kinds, worklist, status, out, prune, tapes, cull, order;
    DevBuf desc, cellrecs, trilist;   // two-pass meshing: per work item / per surface cell / per triangle (sdf_device.h ItemDesc)
    DevBuf blockidx;                  // ... and per 256 triangles of the soup: the work item of the first of them
    bool pruned = false;
    hipStream_t stream = nullptr;  // the stream the generating call ran on (the context's, or a call slot's lane)
    DevBuf counters;               // this call's MeshCounters block (pooled in the context)
    int work_begin = 0, work_end = 0;
    void *emitted_to = nullptr;    // caller buffer the soup was gathered into by sdf_generate_to_device
    // sdf_generate_to_device_async: everything sdf_mesh_wait needs to finish the call
    struct Pending {
        bool active = false;
        GenCall call;                  // (its axes point into `axes`)
        std::vector<double> axes;      // host copy (a soup that does not fit is re-run synchronously)
        CallState got;
    } pend;
    sdfk::DevBlock weld_pts, weld_inv;   // sdf_mesh_weld: unique rows (float64 x 3) / row -> unique row (int64), made by sdf_weld.hip
    long long weld_n = -1;
    // sdf_mesh_vertex_normals: weld_n x 3 float64 + the flat counter in one block of its own (freed with the mesh); the
    // model (content hash) and eps they were taken with: a second call with the same ones reuses them
    sdfk::DevBlock nrm;
    bool nrm_valid = false;
    unsigned long long nrm_model = 0;
    double nrm_eps = 0.0;
    long long nrm_flat = 0;
    // sdf_mesh_components: the shells of the welded mesh -- per vertex, per triangle, the counts and the boxes -- in one block of its
    // own (sdf_components.h ShellParts; freed with the mesh); n_shells >= 0: labelled, a second call reuses them
    sdfk::DevBlock shells;
    long long n_shells = -1;
    int shell_rounds = 0;
    double shell_ms[2] = {0.0, 0.0};
    // sdf_generate_records: the triangles were written as 16-byte records into a slab of the library's (sdf_slab.h); the float64 soup
    // is made on the host threads (sdf_mesh_emit_host_workers) or, for the readers that want it on the device, by k_expand on demand
    bool records = false;
    DevBuf slab;
    long long slab_items = 0, slab_tris = 0, n_raw = 0;
    bool rec_overflow = false;     // the slab (or its raw area) was too small: rec_need_tris is the capacity that holds the call
    long long rec_need_tris = 0;
};

// The grid of a call: batches of bs cells per axis, without the device copies of the axes.  Returns the number of batches; a
// batch size below 1 (sdf_generate_records asks before the batch size has been validated) gives a grid without batches.
inline long long grid_desc(int nx, int ny, int nz, int bs, GridDesc &g) {
    g = GridDesc{};
    g.nx = nx; g.ny = ny; g.nz = nz; g.bs = bs;
    if (bs < 1) return 0;
    g.nbx = (nx + bs - 1) / bs; g.nby = (ny + bs - 1) / bs; g.nbz = (nz + bs - 1) / bs;
    return (long long)g.nbx * g.nby * g.nbz;
}

// the part of a call descriptor that every entry point takes as arguments
inline GenCall gen_call(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs, int sparse,
                        int64_t shard_index, int64_t shard_count, int precision) {
    GenCall call;
    call.tape = t; call.X = X; call.Y = Y; call.Z = Z; call.nx = nx; call.ny = ny; call.nz = nz;
    call.bs = bs; call.sparse = sparse; call.precision = precision; call.shard_index = shard_index; call.shard_count = shard_count;
    return call;
}

// ---- sdf_prepass.hip (k_skip, k_prune_list, k_cull and their launches) ----
int enqueue_skip(sdf_tape *t, const double *d_axes, int nx, int ny, int nz, int bs, int b0, int b1, int precision,
                 unsigned char *d_kinds, hipStream_t st);
int enqueue_prepass(const GenCall &call, sdf_mesh *m, int nb, int tape_stride, hipStream_t st);
int enqueue_cull(sdf_tape *t, sdf_mesh *m, int nb, int tape_stride, bool tail_order, int tail_max, hipStream_t st);
// ---- sdf_eval.hip (k_eval_*) ----
struct FieldTile;   // (sdf_plain.h)
void enqueue_eval_tiles(sdf_tape *t, int precision, const double *dX, const double *dY, const double *dZ, const FieldTile *d_tiles,
                        const int *d_org, float *d_vol, size_t largest_tile, int nt, hipStream_t st);
// ---- sdf_generate.hip (the generate pipeline) ----
int grid_batches(int nx, int ny, int nz, int bs, const char *who, GridDesc &g, int &nb);
int generate_impl(sdf_mesh *m, const GenCall &call);
int finish_call(sdf_mesh *m, const GenCall &call, const CallState &s, bool stats_if_short, sdfk::MeshCounters &h);
// ---- sdf_chunked.hip (batch_size > 32: through device memory, a chunk of batches per submission) ----
int generate_big(sdf_mesh *m, const GenCall &call);
// ---- sdf_mesh_out.hip, and what it shares with the other reader of a finished mesh, sdf_probe_out.hip ----
int copy_to_host(sdf_ctx *c, void *h_dst, const void *d_src, size_t bytes);
// every reader of a mesh first collects a call that is still in flight
#define MESH_READY(m) do { if ((m)->pend.active && sdf_mesh_wait((m), nullptr)) return 1; } while (0)

// where the soup of a mesh lives: the caller's buffer of sdf_generate_to_device, or the library's
static inline const void *mesh_soup(const sdf_mesh *m) { return m->emitted_to ? m->emitted_to : m->out.p; }

// a mesh of sdf_generate_records holds 16-byte records; a reader that wants the float64 soup on the device gets it from k_expand, once
int ensure_soup(sdf_mesh *m);
#define MESH_SOUP_READY(m) do { if (ensure_soup(m)) return 1; } while (0)

// the refusals every entry that takes build directions shares; 0 when the arguments are in order, else 1 with the message set
int overhang_refused(const char *who, const double *h_dirs, long long n_dirs, double sin_limit, double bed_tol);

// the mesh an entry derives from `from` (a selection, a simplified, mended or snapped mesh): like an adopted soup for every reader, but
// it OWNS the soup -- `out` goes back to the pool with the mesh
static inline sdf_mesh *derived_mesh(const sdf_mesh *from, const DevBuf &soup, int64_t n_triangles) {
    sdf_mesh *d = new sdf_mesh();
    d->ctx = from->ctx;
    d->out = soup;
    d->st.n_triangles = n_triangles;
    return d;
}
// ---- sdf_weld.hip: pts = n rows of 3 doubles on the device; on success *d_uniq holds 3 * *n_unique doubles and *d_inv n int64; a
// failed call leaves both empty.  0, or 1 with the message set ----
namespace sdfk {
int weld_device(hipStream_t stream, const double *pts, long long n, DevBlock *d_uniq, DevBlock *d_inv, long long *n_unique);
}
