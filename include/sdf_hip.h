/*
 * sdf_hip.h -- C ABI of libsdf_hip.so, the MI355X (gfx950) sampling + meshing engine.
 *
 * The reference (fogleman/sdf) is a single Python process with no FFI boundary; the seams
 * this ABI replaces are the module-level functions of reference sdf/core.py (cited per entry
 * point).  The host side that binds these symbols is sdf_amd/engine.py (ctypes); the
 * maintainer-side binding is shown in INTEGRATION.md.
 *
 * Conventions: plain C types only; every function returns 0 on success and a non-zero code on
 * failure, with a thread-local message available from sdf_last_error(); no C++ exception crosses
 * the boundary.  Handles are opaque.  A context owns one HIP stream (or adopts the caller's) and
 * all device scratch; calls on one context must not overlap in time (one caller per context);
 * different contexts (e.g. one per GPU / per process) are independent.
 * "host" pointers are ordinary pageable memory, "device" pointers are HIP device memory on the
 * context's GPU.
 */
#ifndef SDF_HIP_H
#define SDF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDF_ABI_VERSION 17

#define SDF_PRECISION_F64 0 /* float64 evaluation like the reference's NumPy path: what every sdf_generate* entry point samples in */
#define SDF_PRECISION_F32 1 /* float32 evaluation: sdf_eval_* and sdf_estimate_bounds only (the meshing path refuses it since round 5) */

typedef struct sdf_ctx sdf_ctx;   /* one HIP device + stream + scratch arenas            */
typedef struct sdf_tape sdf_tape; /* a lowered model (op tape + constants) on the device */
typedef struct sdf_mesh sdf_mesh; /* the result of one sdf_generate call                 */

/* per-call statistics; the first four are what reference sdf/core.py:144-145 prints */
typedef struct sdf_stats {
    int64_t n_batches;
    int64_t n_skipped;
    int64_t n_empty;            /* within this call's shard */
    int64_t n_nonempty;         /* within this call's shard */
    int64_t n_triangles;        /* within this call's shard */
    int64_t n_grid_voxels;      /* len(X)*len(Y)*len(Z)                                    */
    int64_t n_eval_voxels;      /* samples evaluated by the meshing kernel (this shard)    */
    int64_t n_ambiguous_cells;  /* surface cells with an ambiguous sign configuration (the ones Lewiner's tests tile), this
                                 * shard's: counted by k_mesh, and by k_field_rows for batch_size > 32 and sdf_generate_field;
                                 * the CPU checker's n_ambiguous                                                   */
    int64_t n_work_begin;       /* this shard's range in the surviving-batch work list     */
    int64_t n_work_end;
    int64_t n_retries;          /* meshing re-runs after a triangle-arena overflow         */
    double ms_prepass;          /* HIP-event times on the context's stream                 */
    double ms_mesh;             /* the fused sample+march kernel alone (last run)          */
    double ms_emit;             /* ordered gather / f64 transform kernel (last emit)       */
    double ms_total;            /* first launch to last kernel of sdf_generate             */
    int64_t n_pruned_instrs;    /* tape instructions the interval prepass removed, summed over the shard's batches */
    int64_t n_batch_instrs;     /* (instructions per tape) x (batches of the shard): the total they come out of    */
    int64_t n_sampled_voxels;   /* of n_eval_voxels, the samples that went through the interpreter (the rest lie in
                                 * cell groups whose interval excludes the surface; in lots of 64)                 */
    double ms_mesh_device;      /* the sample+march kernel by the device's own constant-rate counter: first workgroup's
                                 * start to last workgroup's end (no HIP event, no host in the measurement)        */
    double sclk_mhz;            /* shader clock that kernel ran at (its cycle counter against the constant one)    */
    double t_mesh_first_us;     /* when that kernel's first workgroup started / its last one ended, microseconds on the */
    double t_mesh_last_us;      /* device's constant-rate counter: calls in flight can be laid on ONE time axis          */
    int64_t mesh_kernel;        /* which fused kernel meshed the call (ABI 8): 1 = k_mesh, one workgroup of 1024 threads per
                                 * compute unit; 0 = neither (batch_size > 32, closures, adopted soups) */
} sdf_stats;

int sdf_abi_version(void);
/* what built this library: the compiler's version lines and the interpreters' flags, as csrc/build.sh recorded them (ABI 7) */
const char *sdf_build_info(void);
const char *sdf_last_error(void);
int sdf_device_count(void); /* <= 0 when no HIP device is usable */

/* free / total device memory (hipMemGetInfo) */
int sdf_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes);
/* TEST HOOK: the nth device / pinned-host allocation the library makes from now on fails once (0: off).  The tests
 * walk it through sdf_ctx_create / sdf_tape_create / sdf_generate and check that every error path returns what it
 * had taken (tests/test_gpu.py::test_failed_allocations_leak_nothing). */
int sdf_test_fail_alloc(int nth);

int sdf_ctx_create(int device, sdf_ctx **out);
int sdf_ctx_destroy(sdf_ctx *ctx);
/* adopt a caller-owned hipStream_t (e.g. torch's current stream); NULL returns to the own stream */
int sdf_ctx_set_stream(sdf_ctx *ctx, void *hip_stream);
/* the interval prepass of sdf_generate (see sdf_tape_set_prune_info) is on by default; 0 switches it
 * off for this context (results are identical either way; the environment variable SDF_PRUNE=0
 * sets the initial state) */
int sdf_ctx_set_prune(sdf_ctx *ctx, int enabled);
/* the same for the second interval pass of sdf_generate: inside a batch, groups of 4^3 cells whose
 * interval excludes the surface are not sampled (SDF_CULL=0 sets the initial state; results are
 * identical either way) */
int sdf_ctx_set_cull(sdf_ctx *ctx, int enabled);
/* how sdf_generate meshes: 0 = one kernel (ordered look-back + parking inside the sampling kernel), 1 = three kernels
 * (sample + classify / number the triangles / emit), -1 = the library's choice by the tape's length (default; the
 * environment variable SDF_MESH_TWOPASS sets the initial state).  Results are identical either way. */
int sdf_ctx_set_twopass(sdf_ctx *ctx, int mode);
/* Inside the one-kernel scheme: 1 (default; SDF_DEFER sets the initial state) = a culled batch keeps only the samples the
 * interval pass listed (a sparse tile) and STAYS in the CU's LDS while the workgroup samples its next batch, so that its
 * triangles are written once, in their final place, when the earlier batches' counts are known; 0 = dense tiles, a
 * batch whose predecessors are not counted yet is parked in device memory and moved later (the r03 scheme).  Results are
 * identical either way. */
int sdf_ctx_set_defer(sdf_ctx *ctx, int on);
/* interval levels of the second interval pass: 2 = boxes of 8^3 and groups of 4^3 cells, 3 = + sub-groups of 2^3 cells,
 * 0 = the library's choice by the tape (default; SDF_CULL_LEVELS sets the initial state).  Results are identical. */
int sdf_ctx_set_cull_levels(sdf_ctx *ctx, int levels);
/* Scheduling of the meshing pass: 1 (default; SDF_TAIL_ORDER sets the initial state) = the last few hundred surviving
 * batches are handed to the workgroups by descending cost estimate instead of by position (shorter tail of the
 * kernel), 0 = strictly in list order.  Results are identical either way. */
int sdf_ctx_set_tail_order(sdf_ctx *ctx, int on);
int sdf_ctx_synchronize(sdf_ctx *ctx);
/* give the device memory the library caches for reuse back to the driver (between jobs of very different sizes) */
int sdf_ctx_trim(sdf_ctx *ctx);

/* Upload an op tape produced by sdf_amd/tape.py (2 x uint32 per instruction, float64 constants).
 * Plays the role of the reference's closure tree (reference sdf/d3.py:48-63). */
int sdf_tape_create(sdf_ctx *ctx, const uint32_t *code, uint32_t n_words, const double *consts,
                    uint32_t n_consts, uint32_t n_pslots, uint32_t n_dslots, sdf_tape **out);
/* Optional: per instruction, where the right operand and the left operand chain of a hard
 * min / max combine start (0xFFFF: not a combine) -- produced by sdf_amd/tape.py next to the tape.
 * With it, sdf_generate runs an interval prepass per surviving batch and skips the instructions
 * that provably cannot influence any sample of that batch (results are unchanged bit for bit). */
int sdf_tape_set_prune_info(sdf_tape *tape, const uint16_t *rstart, const uint16_t *lstart, uint32_t n_instr);
/* 0: sdf_generate runs no interval pass for this tape (neither the instruction pruning nor the cell-group culling).
 * sdf_amd/tape.py asks for that when a constant of the tape is NaN or infinite or makes a divisor of an op zero: such a
 * model is NaN at every sample, which an interval cannot say once a clip or a min / max with a finite operand follows. */
int sdf_tape_set_intervals(sdf_tape *tape, int enabled);
int sdf_tape_destroy(sdf_tape *tape);

/* f(P) for N points of dimension dim (2 or 3): replaces SDF3.__call__ / SDF2.__call__
 * (reference sdf/d3.py:24-25, sdf/d2.py:23-24).  Output is float64 in both precisions. */
int sdf_eval_points(sdf_tape *tape, const void *d_points, int64_t n, int dim, void *d_out, int precision);
int sdf_eval_points_host(sdf_tape *tape, const double *h_points, int64_t n, int dim, double *h_out,
                         int precision);
/* f on the cartesian product X x Y x Z, first axis slowest: replaces `_cartesian_product` +
 * `sdf(P)` (reference sdf/core.py:20-26, :50-52, :78, :232).  h_out has nx*ny*nz elements. */
int sdf_eval_grid_host(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z,
                       int nz, double *h_out, int precision);

/* Models with user-written closures (the reference's documented extension point: a function decorated with
 * @sdf3 / @op3 returns `f(p)`, NumPy code -- reference README.md:258-295, sdf/d3.py:48-63).  The closure runs on
 * the host, in the user's interpreter; the tape reads its values through L_EXTERN leaves.  f(P) then takes two
 * device passes with the closures in between:
 *   sdf_eval_extern_points_host   h_ext_points[k][i][3] = the point leaf k sees for sample i (n_extern x n x 3)
 *   sdf_eval_points_extern_host   f(P) given h_ext_values[k][i] = closure k at that point      (n_extern x n)
 * The plain entry points refuse such a tape. */
int sdf_tape_extern_count(sdf_tape *tape);
int sdf_eval_extern_points_host(sdf_tape *tape, const double *h_points, int64_t n, int dim, double *h_ext_points,
                                int precision);
int sdf_eval_points_extern_host(sdf_tape *tape, const double *h_points, int64_t n, int dim, const double *h_ext_values,
                                double *h_out, int precision);
/* Triangle mesh -> dense narrow-band signed-distance grid (ABI 11; replaces OpenVDB's createLevelSetFromPolygons +
 * copyToArray in `Mesh.sdf`, reference sdf/mesh.py:64-113).  h_points: n_points x 3 float64, h_tris: n_tris x 3 indices.
 * Voxel (i, j, k) sits at (i, j, k) * voxel_size; its value is float32(min(d, background)), negated when an odd number of
 * triangles cross its +z column below it, with d the exact float64 distance to the nearest triangle and background =
 * float32(half_width_voxels * voxel_size).  The result is the index box of the voxels with
 * |value| < background: its first voxel in out_ijk0, its shape in out_dims, the values in h_out, C order [i][j][k].
 * Synchronous.  Like sdf_marching_cubes_host, when prod(out_dims) > cap_voxels (or h_out is NULL) the dims are reported
 * and nothing is filled: call again with a larger buffer.  The arguments are checked on the host before anything is
 * uploaded (an empty mesh, an index out of range, a non-finite point, voxel_size <= 0, a work grid larger than the free
 * device memory allows): those return 2, other failures 1.  Device memory is allocated for the call and freed before
 * it returns. */
int sdf_mesh_level_set_host(sdf_ctx *ctx, const double *h_points, int64_t n_points, const int32_t *h_tris, int64_t n_tris,
                            double voxel_size, int half_width_voxels, int64_t out_ijk0[3], int64_t out_dims[3], float *h_out,
                            int64_t cap_voxels);
/* Boolean mask -> signed exact Euclidean distance texture in pixels (ABI 12; replaces the two scipy
 * distance_transform_edt calls of `text` / `image`, reference sdf/text.py:77-87).  h_mask: rows x cols bytes, C order,
 * non-zero = True; h_out: rows x cols float64.  With D(p) the smallest (d row)^2 + (d col)^2 to a pixel of the OTHER class
 * (an integer), h_out[p] = -sqrt((double)D(p)) where the mask is True and +sqrt((double)D(p)) elsewhere, the square root
 * correctly rounded.  Synchronous.  Refused on the host before anything is uploaded or launched,
 * with return value 2: a NULL pointer, rows or cols below 1, rows^2 + cols^2 >= 2^31 (the squared distances are 32-bit),
 * a shorter side above 16384 pixels, a mask that needs more device memory than is free (13 bytes per pixel), and a mask
 * whose pixels are all of one class.  Other failures return 1.  Device memory is allocated for the call and freed before
 * it returns. */
int sdf_distance_texture_host(sdf_ctx *ctx, const uint8_t *h_mask, int64_t rows, int64_t cols, double *h_out);
/* Sphere-traced render buffers of a model (ABI 13; DESIGN.md section 4e, defined by tests/render_ref.py and reproduced bit for
 * bit).  frame18 = o0, ou, ov, c, du, dv (3 doubles each): pixel (row j, column i) has the origin (o0 + i ou) + j ov and the
 * direction ((c + i du) + j dv) normalised -- a perspective camera has ou = ov = 0, an orthographic one du = dv = 0.
 * params5 = t_near, t_far, hit_eps, step_scale, normal_eps.  A ray marches t += f * step_scale from t_near until f < hit_eps
 * (a hit), t > t_far, f is NaN (misses) or max_steps evaluations are spent (a miss); a hit that stepped inside the surface is
 * bisected back `refine` times; the normal is the normalised central difference of f at the hit, step normal_eps.  Outputs,
 * row-major height x width: h_depth float64 (the hit's ray parameter, +inf for a miss), h_normal 3 x float64 (0 for a miss),
 * h_steps int32 (evaluations of the march), h_status uint8 (1 hit, 0 miss).  Float64 only.  Synchronous, on the context's
 * stream; one device allocation (37 bytes per pixel), freed before it returns; nothing is kept in the context.  Refused on the
 * host before anything is allocated or launched, with return value 2: a NULL pointer, width or height below 1, more than 2^26
 * pixels, max_steps < 1, refine < 0, a non-finite frame or parameter, hit_eps <= 0, normal_eps <= 0, step_scale outside
 * (0, 1], t_far < t_near, and a tape with user closures (sdf_tape_extern_count > 0: every step would need a host round trip).
 * Other failures return 1. */
int sdf_render_host(sdf_tape *tape, const double *frame18, int width, int height, const double *params5, int max_steps, int refine,
                    double *h_depth, double *h_normal, int32_t *h_steps, uint8_t *h_status);
/* the kernel of this thread's last successful sdf_render_host alone, milliseconds by HIP events (tools/render_time.py) */
double sdf_render_last_kernel_ms(void);

/* The batch loop of `generate` (reference sdf/core.py:114-141) around a field evaluated by a HOST callback:
 * `field(user, points (n x 3 float64, host), n, values (n float64, host))` returns 0, or non-zero to abort.  The
 * library builds the points of the skip test (`_skip`, core.py:28-43) and of every surviving batch
 * (`_cartesian_product`, core.py:20-26), calls the field, and meshes the values on the device (float32 cast,
 * marching cubes, `points * scale + offset`); the result is an ordinary sdf_mesh. */
typedef int (*sdf_field_fn)(void *user, const double *points, int64_t n, double *values);
int sdf_generate_field(sdf_ctx *ctx, sdf_field_fn field, void *user, const double *X, int nx, const double *Y, int ny,
                       const double *Z, int nz, int batch_size, int sparse, int64_t shard_index, int64_t shard_count,
                       sdf_mesh **out);

/* `_estimate_bounds` (reference sdf/core.py:62-82: up to 32 rounds of a 16^3 probe grid shrinking from +-1e9) in one
 * launch: h_out6 = x0, y0, z0, x1, y1, z1.  Fails -- with NumPy's message -- where the reference raises (a round in
 * which no probe lies within half a cell diagonal of the surface). */
int sdf_estimate_bounds(sdf_tape *tape, double *h_out6, int precision);

/* Marching cubes of a C-order float32 volume (n0,n1,n2) at level 0: replaces `_marching_cubes`
 * (reference sdf/core.py:16-18 -> skimage.measure.marching_cubes(volume, 0)).  Writes up to
 * cap_tris triangles (9 float32 each: 3 vertices in volume index coordinates, reference soup
 * order) and always reports the full count in *n_tris (call again with a larger buffer if it
 * exceeds cap_tris).  A volume with no surface yields *n_tris == 0 (the reference turns the
 * corresponding skimage exceptions into an empty batch, sdf/core.py:53-56). */
int sdf_marching_cubes(sdf_ctx *ctx, const void *d_volume, int n0, int n1, int n2, void *d_out_tris,
                       int64_t cap_tris, int64_t *n_tris);
int sdf_marching_cubes_host(sdf_ctx *ctx, const float *h_volume, int n0, int n1, int n2, float *h_out_tris,
                            int64_t cap_tris, int64_t *n_tris);

/* The batch loop of `generate` (reference sdf/core.py:114-141) with `_worker` (:45-60) and
 * `_skip` (:28-43) inside: X, Y, Z are the float64 `np.arange` axes (host), batch_size the
 * reference's BATCH_SIZE (1 .. 512; the reference takes any, core.py:87, 114-119), sparse its
 * `sparse=` flag.  shard_index/shard_count split the surviving-batch work list into contiguous
 * chunks (1 GPU: 0, 1).  The triangles stay on the device in the returned mesh until emitted.
 * batch_size <= 32 (the default: 32) runs the fused LDS-resident kernels; a larger batch's
 * (batch_size + 1)^3 float32 tile does not fit a compute unit's LDS and goes through device
 * memory, a chunk of batches per submission, synchronously, into library memory: the variants
 * below that take a caller buffer then report it as not filled (*emitted = 0), exactly as for a
 * buffer that is too small; sdf_generate_compact_async / sdf_generate_from_kinds (the multi-GPU
 * exchange) refuse batch_size > 32. */
int sdf_generate(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                 int batch_size, int sparse, int64_t shard_index, int64_t shard_count, int precision,
                 sdf_mesh **out);
/* The same, writing the ordered soup (`points * scale + offset`, reference sdf/core.py:58-60, :141)
 * straight into caller-owned DEVICE memory of 9*cap_tris doubles.  *emitted = 1 when the soup
 * (sdf_mesh_triangles() triangles) is in d_out; 0 when it did not fit: nothing is written past
 * cap_tris, the contents of d_out are then unspecified, and the mesh holds the complete soup in
 * library memory (the meshing pass was repeated) -- fetch it with sdf_mesh_emit_device/_host. */
int sdf_generate_to_device(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                           int batch_size, int sparse, int64_t shard_index, int64_t shard_count, int precision,
                           void *d_out, int64_t cap_tris, int *emitted, sdf_mesh **out);
/* The same without the host synchronisation: the call is enqueued on the context's stream and the mesh
 * is returned "in flight"; sdf_mesh_wait (or any function that reads the mesh) collects it.  Up to 8
 * calls of one context may be in flight (a ninth waits for the oldest); give each its own d_out.  This
 * is how a caller that meshes many jobs back to back (bench.py) keeps the device busy while the host
 * prepares the next submission; the reference has no counterpart (its generate() is synchronous).
 * sdf_mesh_wait: *emitted as for sdf_generate_to_device (0: the soup did not fit d_out, the call was
 * repeated into library memory). */
int sdf_generate_to_device_async(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                                 int batch_size, int sparse, int64_t shard_index, int64_t shard_count, int precision,
                                 void *d_out, int64_t cap_tris, sdf_mesh **out);
int sdf_mesh_wait(sdf_mesh *mesh, int *emitted);
/* `generate` for a caller who wants the soup ON THE HOST -- the list of points the reference's generate() returns
 * (reference sdf/core.py:131-141): like sdf_generate (one device, the whole work list), but the triangles are written as
 * 16-byte records into a slab of the library's (the exchange unit below: marching cubes' local float32 coordinates + one
 * transform per work item) instead of as 72-byte float64 triangles, and sdf_mesh_emit_host_workers makes the float64 soup
 * on host threads while the records arrive: 47 MB over PCIe instead of 212 MB at 512^3, the same bits (it performs
 * k_expand's `double(local) * scale + offset` on the same operands).  The slab is sized from the last call of the same
 * model on the same grid; the first such call, batch_size > 32 and tapes with user closures are served by sdf_generate.
 * Every reader of the mesh works: those that need the float64 soup on the device get it from k_expand on demand. */
int sdf_generate_records(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                         int batch_size, int sparse, int precision, sdf_mesh **out);
/* Multi-GPU exchange (north_star: "batches shard naturally over the 8 GPUs of one node with an RCCL all-gather of
 * triangle buffers"; the reference itself has no distributed path).  A rank meshes its shard of the surviving-batch
 * work list into a SLAB of fixed capacity in caller-owned device memory -- header (counts, statistics, overflow
 * flag), per-work-item triangle prefix and transform, and the triangles as 16-BYTE records (the three along-edge float32
 * of marching cubes' local coordinates bit for bit + one word for the cell and the edges; a triangle with a vertex inside
 * a cell keeps its nine floats in a small raw area: sdf_amd/csrc/sdf_slab.h, restated in sdf_amd/slabcodec.py) instead of
 * the 72 bytes of the float64 soup -- the caller all-gathers the equal-sized slabs of all
 * ranks in ONE collective, and sdf_expand_slabs writes the ordered float64 soup from the gathered slabs (given in
 * final order) on every rank.  Everything is only ENQUEUED on the context's stream; the caller reads the 128-byte
 * headers (int64[16]: n_tris, n_items, overflow, n_empty, n_nonempty, n_eval, n_ambiguous, n_sampled, n_pruned,
 * n_work_total, n_raw, need_tris, ...) once at the end; overflow != 0 anywhere: repeat with capacities >= the largest
 * n_items and max(n_tris, need_tris). */
size_t sdf_slab_bytes(int64_t cap_items, int64_t cap_tris);
int sdf_generate_compact_async(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                               int batch_size, int sparse, int64_t shard_index, int64_t shard_count, int precision,
                               void *d_slab, int64_t cap_items, int64_t cap_tris, sdf_mesh **out);
int sdf_expand_slabs(sdf_ctx *ctx, const void *const *d_slabs, int n_slabs, int64_t cap_items, int64_t cap_tris,
                     void *d_out, int64_t cap_out_tris);
/* The multi-GPU step inside the library: one process per GPU, RCCL (dlopen'ed: librccl.so.1) over xGMI.
 *   sdf_comm_available   1 if librccl could be loaded in this process, else 0 (sdf_last_error says why).  Local and cheap:
 *                        the ranks agree on it BEFORE anything collective is started, so that a rank without the
 *                        library does not leave the others inside ncclCommInitRank
 *   sdf_comm_unique_id   rank 0 draws one 128-byte id per lane (ncclGetUniqueId) and hands them to the other ranks out
 *                        of band (sdf_amd/dist.py: through the process group that launched the ranks)
 *   sdf_comm_create      collective: every rank, same ids, its own rank.  A communicator has 1 or 2 LANES -- a lane is
 *                        an RCCL communicator + streams + persistent slab / gathered-slab / soup buffers -- so that two
 *                        steps can be in flight: step i + 1 meshes while step i's all-gather is on the links.
 *   sdf_generate_sharded_async   enqueue one step on a lane: mesh this rank's share of the surviving-batch work list
 *                        (contiguous, `chunks` shards per rank; from SDF_SKIP_SHARD_MIN = 32768 batches on the skip
 *                        test itself is shared out too and its one-byte verdicts all-gathered) into slabs, ONE
 *                        ncclAllGather per shard, sdf_expand_slabs' kernel, the gathered headers to pinned memory.
 *                        Nothing waits on the host.  Every rank must submit the same steps in the same order.
 *   sdf_exchange_wait    the step's ONE host synchronisation: reads the gathered headers; slabs that were too small
 *                        are flagged there -- every rank sees the same headers and repeats the step with the
 *                        capacities the headers ask for (first call of a job: a guess, later calls: what the last one
 *                        needed).  *d_soup = the complete ordered float64 soup (9 doubles per triangle, reference
 *                        order: sdf/core.py:141) in library memory on THIS rank's GPU, valid until the next step is
 *                        submitted on the same lane; identical on every rank and to the single-GPU soup. */
#define SDF_COMM_ID_BYTES 128
typedef struct sdf_comm sdf_comm;
typedef struct sdf_exchange sdf_exchange;
typedef struct sdf_exchange_stats {
    int64_t n_batches, n_skipped, n_empty, n_nonempty, n_triangles, n_grid_voxels, n_eval_voxels, n_ambiguous_cells,
        n_sampled_voxels, n_pruned_instrs;      /* whole job (sums over the ranks' slabs)                             */
    int64_t n_retries, chunks, world, slab_bytes;
    double ms_mesh, ms_exchange, ms_expand, ms_total;   /* this rank, HIP events on the lane: prepass + meshing of its
                                                 * shard(s) / until the last all-gather has landed / k_expand / all   */
    int64_t per_rank_triangles[64];
} sdf_exchange_stats;
int sdf_comm_available(void);
int sdf_comm_unique_id(void *out_id128);
int sdf_comm_create(sdf_ctx *ctx, const void *ids, int n_lanes, int rank, int world, sdf_comm **out);
int sdf_comm_destroy(sdf_comm *comm);
int sdf_generate_sharded_async(sdf_comm *comm, sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z,
                               int nz, int batch_size, int sparse, int precision, int chunks, int lane, sdf_exchange **out);
int sdf_exchange_wait(sdf_exchange *x, void **d_soup, int64_t *n_tris);
int sdf_exchange_stats_get(sdf_exchange *x, sdf_exchange_stats *out);
int sdf_exchange_destroy(sdf_exchange *x);
/* `_skip` (reference sdf/core.py:28-43) alone, for batches [b_begin, b_end) of the grid: d_kinds (device memory, one
 * byte per batch of the WHOLE grid) receives 0 (skipped) / 255 (to be meshed) at those positions.  And `generate` for a
 * grid whose verdicts are already there (every byte of d_kinds set): what the sharded step does between its ranks. */
int sdf_skip_kinds(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int batch_size,
                   int64_t b_begin, int64_t b_end, int precision, void *d_kinds);
int sdf_generate_from_kinds(sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                            int batch_size, int64_t shard_index, int64_t shard_count, int precision, const void *d_kinds,
                            sdf_mesh **out);
/* device -> host copy on the context's stream (for soups in library memory: sdf_exchange_wait) */
int sdf_memcpy_to_host(sdf_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int sdf_mesh_stats(sdf_mesh *mesh, sdf_stats *out);
int64_t sdf_mesh_triangles(sdf_mesh *mesh);
/* write the (3T,3) float64 world-space soup (reference order; `points * scale + offset`,
 * reference sdf/core.py:58-60) into caller-owned device / host memory of 9*T doubles */
int sdf_mesh_emit_device(sdf_mesh *mesh, void *d_out);
int sdf_mesh_emit_host(sdf_mesh *mesh, double *h_out);
/* the same with the reference's `workers=` (sdf/core.py:87, 131): the number of host threads that expand the records of a
 * mesh of sdf_generate_records into the float64 soup (<= 0: the machine's, at most 32; a caller's number: at most 64); ignored by any other mesh, whose
 * soup is copied as it is.  sdf_mesh_emit_host = workers 0. */
int sdf_mesh_emit_host_workers(sdf_mesh *mesh, double *h_out, int workers);
/* triangles [first_tri, first_tri + n_tris) of the soup only (9 doubles each) */
int sdf_mesh_emit_host_range(sdf_mesh *mesh, int64_t first_tri, int64_t n_tris, double *h_out);
/* n_batches + 1 entries: h_out[b] = index (within this shard's soup) of the first triangle of batch b in
 * reference batch order, h_out[n_batches] = sdf_mesh_triangles(); batches that were skipped, are empty
 * or belong to another shard have h_out[b] == h_out[b + 1].  This is the bookkeeping the reference keeps
 * implicitly by extending its point list batch after batch (reference sdf/core.py:137-141). */
int sdf_mesh_batch_offsets(sdf_mesh *mesh, int64_t *h_out);
/* T binary-STL records of 50 bytes (f32 normal, 3 x f32 vertex, u16 0), i.e. the body that
 * `write_binary_stl` writes after the 84-byte header (reference sdf/stl.py:4-24) */
int sdf_mesh_emit_stl_host(sdf_mesh *mesh, void *h_out);
/* Vertex weld on the device: what `np.unique(points, axis=0, return_inverse=True)` computes for the
 * reference's non-STL export (reference sdf/core.py:160-164, `_mesh`).  sdf_mesh_weld sorts and
 * deduplicates the soup rows in library memory and reports the number of unique rows;
 * sdf_mesh_weld_fetch copies them out: h_points = n_unique x 3 float64 in lexicographic order,
 * h_cells = T x 3 int64, the unique-row index of every soup row. */
int sdf_mesh_weld(sdf_mesh *mesh, int64_t *n_unique);
/* A mesh handle over a float64 soup that ALREADY sits in device memory (n_tris x 9 doubles, e.g. the gathered soup of a
 * multi-GPU step): sdf_mesh_emit_stl_host / sdf_mesh_weld / sdf_mesh_emit_host* then work on it like on a soup the
 * library generated.  The memory stays the caller's (alive and complete until the handle is destroyed). */
int sdf_mesh_adopt_soup(sdf_ctx *ctx, const void *d_soup, int64_t n_tris, sdf_mesh **out);
int sdf_mesh_weld_fetch(sdf_mesh *mesh, double *h_points, int64_t *h_cells);
/* Vertex normals of the welded mesh from the FIELD (ABI 14; DESIGN.md section 4f, defined by tests/normals_ref.py and reproduced
 * bit for bit): at every unique vertex p of sdf_mesh_weld, for axis k = 0, 1, 2, g_k = f(p + eps e_k) - f(p - eps e_k) (only
 * coordinate k changes, by x + eps and x + (-eps)), len = sqrt((g0*g0 + g1*g1) + g2*g2), n = g / len; a vertex whose len is 0 or
 * NaN is "flat": its normal is (0, 0, 0) and it is counted in *n_flat.  Float64, the interpreter of sdf_eval_points.  The normals
 * (n_unique x 3 float64) stay on the device with the mesh, until it is destroyed, and are copied to h_normals unless it is NULL; a
 * second call with the same model and eps reuses them.  The tape is an argument so that adopted soups (sdf_mesh_adopt_soup) are
 * served.  Refused on the host before anything is allocated or launched, with return value 2: a NULL mesh, tape or n_flat, an eps
 * that is not finite or not above 0, a tape with user closures (sdf_tape_extern_count > 0), a mesh that is not welded, a tape of
 * another context.  Other failures return 1. */
int sdf_mesh_vertex_normals(sdf_mesh *mesh, sdf_tape *tape, double eps, double *h_normals, int64_t *n_flat);
/* the kernel of this thread's last sdf_mesh_vertex_normals that computed (not one served from the cache) alone, milliseconds by
 * HIP events (tools/export_time.py) */
double sdf_mesh_normals_last_kernel_ms(void);
/* The wall thickness at the welded vertices (added under ABI 17: the version is unchanged, nothing above changes; DESIGN.md section
 * 4l, defined by tests/thickness_ref.py and reproduced bit for bit): from every unique vertex p of sdf_mesh_weld a ray is
 * sphere-traced INWARD through the solid until the field f turns positive again.  params6 = normal_eps, start, min_step, t_far,
 * step_scale, 0 (reserved).  The direction is d = -(g / len) with g, len of sdf_mesh_vertex_normals at step normal_eps; a vertex
 * whose len is 0 or NaN is FLAT (3): thickness NaN, 0 steps.  The march starts at t = start with the bracket lo = 0, hi = start
 * and evaluates v = f(p + t d) at most max_steps times: a NaN ends it as NAN (4, thickness NaN); v >= 0 ends it with hi = t -- on
 * the first evaluation as THIN (2: nothing solid lies `start` inside the vertex; the thickness reported is `start`, an upper
 * bound), later as THICK (1); otherwise lo = t and t advances by max((-v) * step_scale, min_step), and a t beyond t_far ends it
 * as OPEN (0, thickness +inf), as does running out of steps.  The bracket of a THICK vertex is bisected `refine` times (the
 * midpoint goes to lo where f < 0 there, else to hi) and its thickness is hi.  min_step lets a ray leave the surface it starts on
 * and pass along a nearby face; the price is that an outside gap narrower than min_step can be stepped over.  Outputs, one per
 * welded vertex: h_thickness float64, h_status uint8, h_steps int32 (evaluations of the march).  Float64, the interpreter of
 * sdf_eval_points.  It serves every mesh of the context that has been welded: generated meshes, adopted soups, selections,
 * simplified and mended meshes.  Synchronous, on the context's stream; one device allocation (13 bytes per vertex), freed before
 * it returns; nothing is kept with the mesh.  A mesh of 0 vertices returns 0 without a launch.  Refused on the host before
 * anything is allocated or launched, with return value 2: a NULL argument, a mesh that is not welded, a tape of another context, a
 * tape with user closures (sdf_tape_extern_count > 0), a non-finite parameter, normal_eps, start or min_step not above 0,
 * step_scale outside (0, 1], t_far < start, max_steps < 1, refine < 0.  Other failures return 1. */
int sdf_mesh_vertex_thickness(sdf_mesh *mesh, sdf_tape *tape, const double *params6, int max_steps, int refine,
                              double *h_thickness, uint8_t *h_status, int32_t *h_steps);
/* the kernel of this thread's last successful sdf_mesh_vertex_thickness alone, milliseconds by HIP events (tools/thickness_time.py) */
double sdf_mesh_thickness_last_kernel_ms(void);
/* The curvature of the field's level set at the welded vertices (added under ABI 17: the version is unchanged, nothing above changes;
 * DESIGN.md section 4t, defined by tests/curvature_ref.py and reproduced bit for bit): at every unique vertex p of sdf_mesh_weld the
 * field f is evaluated 19 times -- v0 = f(p); for axis a = x, y, z the values va+, va- at p with coordinate a moved by + eps and by
 * + (-eps); for the pairs (a, b) = (x, y), (x, z), (y, z) the values v++, v+-, v-+, v-- with a moved by +-eps, then b.  From them
 * G_a = (va+ - va-) / (2 eps), H_aa = ((va+ - v0) + (va- - v0)) / (eps eps), H_ab = ((v++ - v+-) - (v-+ - v--)) / ((4 eps) eps);
 * L2 = (Gx Gx + Gy Gy) + Gz Gz, L = sqrt(L2), tr = (Hxx + Hyy) + Hzz, gMg = ((Gx Gx Mxx + Gy Gy Myy) + Gz Gz Mzz) + 2 ((Gx Gy Mxy +
 * Gx Gz Mxz) + Gy Gz Myz) for a symmetric M (products left to right); mean = (L2 tr - gHg) / ((2 L2) L); gauss = gAg / (L2 L2)
 * with A the cofactors of H (Axx = Hyy Hzz - Hyz Hyz, Ayy = Hxx Hzz - Hxz Hxz, Azz = Hxx Hyy - Hxy Hxy, Axy = Hxz Hyz - Hxy Hzz,
 * Axz = Hxy Hyz - Hxz Hyy, Ayz = Hxy Hxz - Hxx Hyz); disc = mean mean - gauss, 0 where it is not > 0; k1 = mean + sqrt(disc),
 * k2 = mean - sqrt(disc).  The field is negative inside, so convex is positive: a sphere of radius R has k1 = k2 = 1 / R, a cavity
 * is negative.  Status, in this order: NAN (2) where one of the 19 values is not finite; FLAT (1) where L2 == 0 or L is not finite;
 * NAN (2) where one of the four results is not finite; else CURVED (0).  A vertex that is not CURVED holds the bits
 * 0x7ff8000000000000 in all four outputs.  Outputs, one per welded vertex: h_curv4 4 x float64 (mean, gauss, k1, k2), h_status
 * uint8; h_counts3: the vertices of status 0, 1, 2.  Float64, the interpreter of sdf_eval_points, one rounding per operation.  It
 * serves every mesh of the context that has been welded, like sdf_mesh_vertex_thickness.  Synchronous, on the context's stream; one
 * device allocation (33 bytes per vertex), freed before it returns; nothing is kept with the mesh.  A mesh of 0 vertices returns 0
 * without a launch.  Refused on the host before anything is allocated or launched, with return value 2: a NULL argument, a mesh
 * that is not welded, a tape of another context, a tape with user closures (sdf_tape_extern_count > 0), an eps that is not finite
 * or not above 0.  Other failures return 1. */
int sdf_mesh_vertex_curvature(sdf_mesh *mesh, sdf_tape *tape, double eps, double *h_curv4, uint8_t *h_status, int64_t *h_counts3);
/* the kernel of this thread's last successful sdf_mesh_vertex_curvature alone, milliseconds by HIP events (tools/curvature_time.py) */
double sdf_mesh_curvature_last_kernel_ms(void);
/* A mesh held to the field (added under ABI 17: the version is unchanged, nothing above changes; DESIGN.md section 4q, defined by
 * tests/deviation_ref.py and reproduced bit for bit).  Float64, the interpreter of sdf_eval_points, one rounding per operation.
 *
 * sdf_mesh_triangle_deviation samples the field f on every triangle (A, B, C) of the float64 soup: order = n in 1 .. 8, the
 * S = (n+1)(n+2)/2 samples in the order for i in 0..n: for j in 0..n-i, weights wa = (n-i-j)/n, wb = i/n, wc = j/n, sample point
 * (A*wa + B*wb) + C*wc per coordinate; sample 0 is corner A.  Per triangle: h_dev float64, the sampled value of largest magnitude
 * (a later sample replaces it only where its magnitude is strictly greater; the first NaN replaces it and stays), h_at int32, that
 * sample's index, h_sumsq float64, the sequential sum of the squared values.  Needs no weld; serves every mesh that has (or can
 * make) a soup on the device.  One device allocation (20 bytes per triangle), freed before it returns.  A mesh of 0 triangles
 * returns 0 without a launch.  Refused on the host before anything is allocated or launched, with return value 2: a NULL argument,
 * a tape of another context, a tape with user closures, order outside 1 .. 8, 2^31 or more triangles.
 *
 * sdf_mesh_snap moves the unique vertices P of sdf_mesh_weld onto the zero set.  params4 = eps, tol, max_move, 0 (reserved).  Every
 * vertex starts at q = P as ITER; in each of `iters` passes a vertex still ITER evaluates v = f(q): NaN makes it NAN (4) and puts q
 * back to P, |v| <= tol makes it SNAPPED (1); otherwise g is the central difference of sdf_mesh_vertex_normals at q with step eps,
 * len2 = (g0*g0 + g1*g1) + g2*g2, zero or NaN makes it FLAT (3) where it is; otherwise s = (v * (2 eps)) / len2, qn = q - s g (the
 * Newton step v grad / |grad|^2), and if |qn - P| > max_move the vertex is HELD (2) where it is, else q = qn.  After the passes a
 * vertex still ITER is SNAPPED if |f(q)| <= tol, else LEFT (0).  The result is a NEW mesh whose soup is q taken through the welded
 * cells, in triangle order and winding; it OWNS its soup, like a simplified mesh, and serves every reader; the source mesh stays
 * valid and unchanged.  Vertices that land on one point make a collapsed triangle (sdf_mesh_mend drops it); topology is not
 * preserved and creases are not restored.  h_points (n_unique x 3 float64), h_status (uint8), h_residual (float64: f at the
 * final q, NaN for NAN) and h_evals (int32: the evaluations the vertex needed -- 1 per pass it entered, 6 more where it took the
 * gradient, 1 for the final value of a vertex still ITER) are in the source's weld order; each may be NULL.  Refused with return value 2: a NULL mesh, tape, params4,
 * out or stats, a mesh that is not welded, a tape of another context, a tape with user closures, a non-finite parameter, eps <= 0,
 * tol < 0, max_move < 0, iters < 1.  Other failures return 1 with nothing left allocated; *out is written on success only. */
typedef struct sdf_snap_stats {
    int64_t vertices, left, snapped, held, flat, nan;
    double kernel_ms;
} sdf_snap_stats;
int sdf_mesh_triangle_deviation(sdf_mesh *mesh, sdf_tape *tape, int order, double *h_dev, int32_t *h_at, double *h_sumsq);
int sdf_mesh_snap(sdf_mesh *mesh, sdf_tape *tape, const double *params4, int iters, sdf_mesh **out, double *h_points,
                  uint8_t *h_status, double *h_residual, int32_t *h_evals, sdf_snap_stats *stats);
/* the kernel of this thread's last successful sdf_mesh_triangle_deviation alone, milliseconds by HIP events (tools/deviation_time.py) */
double sdf_mesh_deviation_last_kernel_ms(void);
/* The body of a binary little-endian PLY file of the welded mesh: h_vertices receives n_unique records of float32 x, y, z (12
 * bytes) or, with_normals = 1, float32 x, y, z, nx, ny, nz (24 bytes; needs a successful sdf_mesh_vertex_normals first);
 * h_faces receives T records of 13 bytes: uint8 3 and three little-endian int32 vertex indices.  Refused with return value 2: a
 * NULL argument, a mesh that is not welded, with_normals without normals, 2^31 or more vertices.  One device allocation, freed
 * before it returns. */
int sdf_mesh_emit_ply_host(sdf_mesh *mesh, int with_normals, void *h_vertices, void *h_faces);
/* The mesh measured on the device (ABI 15; DESIGN.md section 4g, defined by tests/measure_ref.py and reproduced bit for bit).
 * sdf_mesh_moments streams the float64 soup once (after one pass for its bounding box) and returns RAW totals over the triangles
 * (A, B, C), taken relative to a reference point o: a = A - o, b = B - o, c = C - o, n = (b - a) x (c - a), det = a . (b x c),
 * s = a + b + c.  sums[0] = sum |n| (twice the area), sums[1] = sum det (six times the volume), sums[2..4] = sum det s_k (24 times
 * the first moments about o), sums[5..10] = sum det (a_i a_j + b_i b_j + c_i c_j + s_i s_j) for ij = xx, yy, zz, xy, xz, yz (120
 * times the second moments about o).  Every multiply and add is rounded separately, and the sums run through a fixed tree (chunks
 * of 1024 triangles, 256 lanes, halving): the totals depend on the order of the triangles and on nothing else.  origin = 3 doubles,
 * or NULL for the midpoint of the bounding box, lo + (hi - lo) / 2 ((0, 0, 0) for an empty box); the point used comes back in
 * `origin`.  A triangle with a non-finite vertex adds +0.0 to every sum, is left out of the box and is counted in n_nonfinite;
 * n_zero_area counts the others whose |n| is 0.  A zero of the box is +0.0; an empty box (no triangles, or none finite) is
 * lo = +inf, hi = -inf.  Needs no weld; serves every mesh that has (or can make) a soup on the device, adopted ones included.
 * One device allocation, freed before it returns.  A NULL mesh or out returns 2, other failures 1. */
typedef struct sdf_moments {
    double sums[11];
    double origin[3];
    double box_lo[3], box_hi[3];
    int64_t n_triangles, n_zero_area, n_nonfinite;
} sdf_moments;
int sdf_mesh_moments(sdf_mesh *mesh, const double *origin, sdf_moments *out);
/* The edge census of the welded mesh (cells of sdf_mesh_weld): a cell with two equal indices is COLLAPSED (counted, no edges);
 * every other cell gives three directed half-edges, and an undirected edge is PAIRED (two uses, opposite directions), BOUNDARY
 * (one use), MISORIENTED (two uses, one direction) or NONMANIFOLD (three or more uses).  edges = the sum of the four, faces =
 * T - collapsed, vertices = n_unique, euler = vertices - edges + faces, closed = (boundary == 0 and nonmanifold == 0), oriented =
 * (misoriented == 0).  One kernel for the keys, one library radix sort over 3T 64-bit keys, one kernel for the classes; one device
 * allocation (48 bytes per triangle + the sort's), freed before it returns.  Refused on the host before anything is allocated or
 * launched, with return value 2: a NULL argument, a mesh that is not welded, 3T >= 2^31 or 2^31 or more vertices.  Other failures
 * return 1. */
typedef struct sdf_edge_census {
    int64_t vertices, faces, collapsed, edges, paired, boundary, misoriented, nonmanifold, euler, closed, oriented;
} sdf_edge_census;
int sdf_mesh_edge_census(sdf_mesh *mesh, sdf_edge_census *out);
/* the kernels of this thread's last sdf_mesh_moments or sdf_mesh_edge_census alone (box + moments + partials; keys + sort +
 * classes), milliseconds by HIP events (tools/measure_time.py) */
double sdf_mesh_measure_last_kernel_ms(void);
/* The connected shells of the welded mesh (ABI 16; DESIGN.md section 4h, defined by tests/components_ref.py and reproduced exactly).
 * Every cell joins its three welded indices -- a collapsed cell (a, a, b) joins a and b like any other --, the LABEL of a vertex is
 * the smallest welded index of its connected component, and the shells are numbered 0 .. K - 1 by ascending label, that is by their
 * lexicographically smallest vertex.  vertex_shell[v] is the shell of welded vertex v, triangle_shell[t] the shell of the first
 * vertex of cell t; per shell: its triangles, its vertices and the bounding box of its vertices (a zero reads +0.0).  The result is
 * a function of the cells alone: nothing in it depends on launch geometry, timing or the order of atomics.
 * sdf_mesh_components welds first if that has not happened, labels on the device (a 32-bit parent word per vertex: root hooking by
 * compare-and-swap, compression, and a verifying pass over every cell behind a kernel boundary -- `rounds` counts the passes, at most
 * ceil(log2(max(V, 2))) + 2), numbers the roots with a library scan and takes the counts and boxes with integer atomics.  It serves
 * generated meshes, meshes of sdf_generate_records and adopted soups.  The arrays stay on the device in one block of the mesh's own
 * until it is destroyed; a second call reuses them.  One scratch allocation, freed before it returns.  A mesh of 0 triangles has 0
 * shells, and nothing is launched.  ms_label / ms_number: the kernels of the labelling (with the host's look at the counter between
 * the rounds) and of numbering + counts + boxes of the call that computed, by HIP events.  Refused with return value 2: a NULL
 * argument, 2^31 or more triangles or vertices.  Other failures return 1. */
typedef struct sdf_components {
    int64_t n_shells, n_vertices, n_triangles, rounds;
    double ms_label, ms_number;
} sdf_components;
int sdf_mesh_components(sdf_mesh *mesh, sdf_components *out);
/* ... copied out: h_vertex_shell n_vertices x int32, h_triangle_shell n_triangles x int32, h_triangles and h_vertices n_shells x
 * int64, h_bounds n_shells x 2 x 3 float64 (lo x, y, z, hi x, y, z).  Any pointer may be NULL.  Return value 2: a NULL mesh, a mesh
 * that has not been through sdf_mesh_components. */
int sdf_mesh_components_fetch(sdf_mesh *mesh, int32_t *h_vertex_shell, int32_t *h_triangle_shell, int64_t *h_triangles,
                              int64_t *h_vertices, double *h_bounds);
/* A new mesh of the triangles whose shell k has h_keep[k] != 0, in soup order, bit for bit (a flag per triangle, a library scan, one
 * copy kernel).  The new mesh OWNS its soup, which goes back to the library's pool when it is destroyed; for every reader it is what
 * an adopted soup is (sdf_mesh_emit_stl_host, sdf_mesh_weld, sdf_mesh_emit_ply_host, sdf_mesh_vertex_normals, sdf_mesh_moments,
 * sdf_mesh_edge_census, sdf_mesh_emit_host*, and sdf_mesh_components itself).  The source mesh stays valid and unchanged.  Keeping
 * nothing gives a mesh of 0 triangles without a launch.  Refused on the host before anything is allocated or launched, with return
 * value 2: a NULL argument, a mesh that has not been through sdf_mesh_components, n_keep != n_shells.  Other failures return 1, and
 * *out is NULL. */
int sdf_mesh_select_shells(sdf_mesh *mesh, const unsigned char *h_keep, int64_t n_keep, sdf_mesh **out);
/* the kernels of this thread's last sdf_mesh_components that computed (labelling + numbering + counts) or sdf_mesh_select_shells
 * (flags + scan + copy) alone, milliseconds by HIP events (tools/shells_time.py) */
double sdf_mesh_components_last_kernel_ms(void);
/* The mesh simplified on the device (ABI 17; DESIGN.md section 4j, defined by tests/simplify_ref.py and reproduced bit for bit):
 * vertex clustering on the uniform grid (origin3, cell3) -- the cluster of a welded vertex is floor((p - origin) / cell) per axis,
 * clusters are numbered by ascending key x << 42 | y << 21 | z of their cell relative to the smallest one -- with one representative
 * per cluster placed by a quadric error function: the planes of the triangles that touch the cluster, weighted by their squared
 * area, regularised by reg x trace towards the mean of the cluster's vertices, solved in closed form; a representative that is not
 * finite or leaves its cell is replaced by that mean (`mean_fallback`), a cluster of zero-area triangles only takes the mean too
 * (`flat`).  A triangle survives if its three clusters differ; survivors keep their order and winding (`collapsed` counts the
 * others).  Duplicate triangles and oppositely wound pairs are NOT removed unless the result goes through sdf_mesh_mend
 * (sdf_mesh_edge_census reports them), and topology is
 * not preserved.  Every float sum is sequential in the definition's order (one lane per cluster): the result does not depend on
 * launch geometry or the order of atomics.  sdf_mesh_simplify welds the source first if that has not happened; it serves generated
 * meshes, meshes of sdf_generate_records, adopted soups and selections.  The new mesh OWNS its soup, like a selection's, and is what
 * an adopted soup is for every reader; the source mesh stays valid and unchanged.  One scratch allocation, freed before the call
 * returns whether it fails or not.  A mesh of 0 triangles gives a mesh of 0 triangles without a launch.  kernel_ms: the kernels
 * alone, by HIP events.  Refused on the host before anything is allocated or launched, with return value 2: a NULL argument, a
 * cell that is not positive and finite, an origin that is not finite, a reg that is negative or not finite, 2^31 or more corners
 * (3 x triangles) or vertices.  Found after the first pass over the vertices, with return value 1 and nothing left allocated: a
 * vertex that is not finite, clusters that span 2^21 or more cells on an axis.  *out is written on success only. */
typedef struct sdf_simplify_stats {
    int64_t clusters, triangles_in, triangles_out, collapsed, mean_fallback, flat;
    double kernel_ms;
} sdf_simplify_stats;
int sdf_mesh_simplify(sdf_mesh *mesh, const double *origin3, const double *cell3, double reg, sdf_mesh **out, sdf_simplify_stats *stats);
/* the kernels of this thread's last sdf_mesh_simplify, milliseconds by HIP events; parts4 (or NULL): keys and numbering, the item
 * sort and its segments, k_cluster_vertex, live flags and emission (tools/simplify_time.py) */
double sdf_mesh_simplify_last_kernel_ms(double *parts4);
/* The mesh simplified to a tolerance (added under ABI 17: the version is unchanged, nothing above changes; DESIGN.md section 4p,
 * defined by tests/adaptive_ref.py and reproduced bit for bit): octree vertex clustering with the quadric above as the error
 * measure.  Level L = 0 .. levels is sdf_mesh_simplify's clustering on the grid (origin3, cell3 x 2^L).  The error of a cluster is
 * the sum, over the (triangle, corner) items that touch it, of the squared residual of its representative in the triangle's plane
 * (normal of twice-the-area length); the cluster is accepted if err <= tolerance^2 x w, w the trace of its quadric -- the
 * squared-area-weighted mean squared distance of the representative from those planes against tolerance^2; it is not a Hausdorff
 * bound.  Level 0 is always accepted, and every cluster is when tolerance^2 is +inf.  Every welded vertex takes the coarsest level
 * whose cluster is accepted, that cluster's representative as its position and (level, cluster) as its id; a triangle survives if
 * its three ids differ, in order and winding.  levels = 0 is sdf_mesh_simplify bit for bit, and so is tolerance = +inf on the
 * cell x 2^levels.  clusters_used[L], vertices[L]: the clusters of level L that a vertex chose, and those vertices; mean_fallback
 * and flat count the used clusters.  Every float sum is sequential in the definition's order.  One scratch allocation, reused across
 * the levels and freed before the call returns; the new mesh OWNS its soup, like sdf_mesh_simplify's.  A mesh of 0 triangles gives a
 * mesh of 0 triangles without a launch.  Refused on the host with return value 2: what sdf_mesh_simplify refuses, a tolerance that
 * is negative or NaN, levels outside 0 .. SDF_ADAPTIVE_MAX_LEVELS, a cell3 x 2^levels that is not finite.  Found on the device with
 * return value 1 and nothing left allocated: a vertex that is not finite, clusters of a level that span 2^21 or more cells on an
 * axis.  *out is written on success only. */
#define SDF_ADAPTIVE_MAX_LEVELS 10
typedef struct sdf_adaptive_stats {
    int64_t triangles_in, triangles_out, collapsed, levels, mean_fallback, flat;
    int64_t clusters_used[SDF_ADAPTIVE_MAX_LEVELS + 1], vertices[SDF_ADAPTIVE_MAX_LEVELS + 1];
    double kernel_ms;
} sdf_adaptive_stats;
int sdf_mesh_simplify_adaptive(sdf_mesh *mesh, const double *origin3, const double *cell3, double reg, double tolerance, int levels,
                               sdf_mesh **out, sdf_adaptive_stats *stats);
/* the kernels of this thread's last sdf_mesh_simplify_adaptive, milliseconds by HIP events: their sum (the levels and the emission);
 * ms (or NULL): levels + 1 values, one per level (tools/adaptive_time.py) */
double sdf_mesh_simplify_adaptive_last_kernel_ms(double *ms);
/* The mesh mended on the device (added under ABI 17: the version is unchanged, nothing above changes; DESIGN.md section 4k, defined
 * by tests/mend_ref.py and reproduced exactly): duplicate triangles are dropped and oppositely wound pairs cancel -- what
 * sdf_mesh_simplify leaves behind where two sheets of a surface fall into the same clusters.  A cell of the weld with two equal
 * indices is dropped (`collapsed`).  Every other cell, rotated so that its smallest index comes first, (a, b, c), has the face
 * (a, min(b, c), max(b, c)) and the side b > c.  Of the cells of one face, n0 on one side and n1 on the other: n0 == n1 drops all of
 * them (`cancelled`); otherwise one survives, the first in soup order of the majority side, and the others are `duplicates`.
 * `faces` counts the distinct faces.  The survivors keep their order and winding, and their nine doubles are the source soup's, bit
 * for bit.  triangles_in == triangles_out + collapsed + duplicates + cancelled.  Integers only: the result is a function of the
 * welded cells and does not depend on launch geometry or the order of atomics.  NOT done: a misoriented mesh is not re-oriented,
 * and where a thin wall collapsed only in part the rim of the collapsed region stays non-manifold (sdf_mesh_edge_census goes on
 * reporting it).  sdf_mesh_mend welds the source first if that has not happened; it serves generated meshes, meshes of
 * sdf_generate_records, adopted soups, selections and simplified meshes.  The new mesh OWNS its soup, like a selection's, and is
 * what an adopted soup is for every reader; the source mesh stays valid and unchanged.  One scratch allocation (40 bytes per
 * triangle and the library sort's), freed before the call returns whether it fails or not.  A mesh of 0 triangles, or one of which
 * nothing survives, gives a mesh of 0 triangles (the first without a launch).  kernel_ms: the kernels alone, by HIP events.  Refused
 * on the host before anything is allocated or launched, with return value 2: a NULL argument, 2^31 or more corners (3 x triangles;
 * the vertices of a weld are no more than its corners).  Other failures return 1 with nothing left allocated; *out is written on
 * success only. */
typedef struct sdf_mend_stats {
    int64_t triangles_in, triangles_out, collapsed, duplicates, cancelled, faces;
    double kernel_ms;
} sdf_mend_stats;
int sdf_mesh_mend(sdf_mesh *mesh, sdf_mesh **out, sdf_mend_stats *stats);
/* the kernels of this thread's last sdf_mesh_mend, milliseconds by HIP events; parts3 (or NULL): the keys, the two sorts, runs and
 * emission (tools/mend_time.py) */
double sdf_mesh_mend_last_kernel_ms(double *parts3);
/* The contours of a sampled 2-D field: closed, oriented, ordered polylines (added under ABI 17: the version is unchanged, nothing
 * above changes; DESIGN.md section 4m, defined by tests/contour_ref.py and reproduced bit for bit).  Samples V[nw][nx][ny] (nw
 * layers, the last axis fastest) over the axes X[nx], Y[ny]; a sample is inside iff v < level.  Marching squares with the saddles
 * decided by the cell's centre value ((v00 + v10) + (v01 + v11)) * 0.25; a cell emits 0 .. 2 segments with the inside on their
 * left, so outer boundaries run counter-clockwise (positive area) and holes clockwise (negative area); a cell with a non-finite
 * corner emits nothing and is counted.  The vertex of a grid edge is computed from the lower-index sample a to the higher-index
 * one b, t = (a - level) / (a - b), c = ca + t * (cb - ca).  Segments are numbered by layer, cell ix * (ny - 1) + iy and slot, linked
 * through the case table, and every chain is one contour: a closed loop starts at its smallest segment index and has one point per
 * segment, an open chain (it ends at the border of the grid or beside a non-finite cell) starts at its segment without a
 * predecessor and has one point more.  Contours are ordered by that first segment, which groups them by layer.  area is the
 * shoelace sum, left to right from the first point; 0 for an open chain.  Segments of length zero (a sample equal to the level)
 * are kept.
 *   sdf_contour_grid_host   contours of a host sample grid: the twin of sdf_marching_cubes_host, and what serves models with user
 *                           closures and float32 evaluation (the caller evaluates, then calls this).
 *   sdf_contour_host        samples on the device -- float64, the interpreter of sdf_eval_points over points made from the axes, in
 *                           slabs of at most 2^24 -- and contours.  dim 3: layer w lies at z = W[w]; dim 2: W is ignored and nw must
 *                           be 1.  h_values (or NULL) receives the nw * nx * ny samples.
 * Both return a handle and the counts; sdf_contours_fetch copies the arrays out -- h_points n_points x 2 float64, h_offsets
 * (n_contours + 1) int64, h_closed n_contours uint8, h_layer n_contours int32, h_area n_contours float64; any pointer may be NULL --
 * and sdf_contours_destroy frees the handle's one device block.  Synchronous, on the context's stream.  Device memory: two scratch
 * allocations (17 bytes per sample and the library scan's, the slab of points; 60 bytes per segment), freed before the call
 * returns whether it fails or not, and the handle's block.  `rounds` = ceil(log2(n_segments)): the launches of each of the two
 * pointer-jumping phases of the linking.  Refused on the host before anything is allocated or launched, with return value 2: a NULL
 * pointer, nx < 2 or ny < 2, nw < 1, nw * nx * ny > 2^28, a level or an axis value that is not finite, axes that are not strictly
 * increasing, a dim other than 2 and 3, dim 2 with nw != 1, a tape with user closures (sdf_tape_extern_count > 0).  Other failures
 * return 1 and *out is NULL. */
typedef struct sdf_contours sdf_contours;
typedef struct sdf_contour_counts {
    int64_t n_points, n_contours, n_segments, nonfinite_cells, rounds;
} sdf_contour_counts;
int sdf_contour_grid_host(sdf_ctx *ctx, const double *h_values, int nw, int nx, int ny, const double *X, const double *Y, double level,
                          sdf_contours **out, sdf_contour_counts *counts);
int sdf_contour_host(sdf_tape *tape, int dim, const double *X, int nx, const double *Y, int ny, const double *W, int nw, double level,
                     double *h_values, sdf_contours **out, sdf_contour_counts *counts);
int sdf_contours_fetch(sdf_contours *contours, double *h_points, int64_t *h_offsets, uint8_t *h_closed, int32_t *h_layer, double *h_area);
int sdf_contours_destroy(sdf_contours *contours);
/* the kernels of this thread's last sdf_contour_grid_host or sdf_contour_host, milliseconds by HIP events; parts4 (or NULL): the
 * sampling (0 for the grid entry), count + scan + emit, the linking with its scans and the scatter, the areas (tools/contour_time.py) */
double sdf_contour_last_kernel_ms(double *parts4);
/* Build directions rated on the device (added under ABI 17: the version is unchanged, nothing above changes; DESIGN.md section 4n,
 * defined by tests/overhang_ref.py and reproduced bit for bit).  For the float64 soup of a mesh and n_dirs UNIT directions d ("up": the
 * bed lies below the part), per direction: h(p) = (px dx + py dy) + pz dz and its extremes lo, hi over the vertices of the finite
 * triangles (none: +inf, -inf); per triangle (a, b, c) with the raw normal n = (b - a) x (c - a), dbl = |n|, dn = (nx dx + ny dy) +
 * nz dz and ha, hb, hc = h - lo:  on_bed = max(ha, hb, hc) <= bed_tol;  overhang = finite, not on_bed, dn < -(sin_limit * dbl);
 * contact = finite, on_bed, dn < 0.  s0 = sum of dbl over the overhangs (twice their area), s1 = sum of (-dn) ((ha + hb) + hc) over
 * them (six times the volume of the prisms from the overhanging faces straight down to the bed plane -- a PROXY for the support: the
 * part's own material under an overhang is not subtracted, and the faces hidden inside a soup of overlapping solids count), s2 = sum
 * of dbl over the contacts (twice the area on the bed).  Every multiply and add is rounded separately and the sums run through a
 * fixed tree: chunks of 1024 consecutive triangles summed one after the other from +0.0, the chunk partials in groups of 256 through
 * the halving tree of sdf_mesh_moments.  The result does not depend on launch geometry, the order of atomics, or the slabs:
 * the directions are taken in slabs whose chunk partials stay under max_scratch_bytes (0: 64 MiB; never fewer than one direction).
 *   sdf_mesh_overhangs         h_values: n_dirs x 5 float64 (lo, hi, s0, s1, s2); h_counts: n_dirs x 2 int64 (overhanging triangles,
 *                              bed-contact triangles).
 *   sdf_mesh_overhang_classes  one direction h_dir3; h_classes: one byte per triangle -- 0 neither, 1 overhang, 2 bed contact,
 *                              3 non-finite -- by the same predicates.
 * Both serve generated meshes, meshes of sdf_generate_records and adopted soups, like sdf_mesh_moments.  Synchronous, on the
 * context's stream; one scratch allocation, freed before the call returns whether it fails or not.  A mesh of 0 triangles gives the
 * empty result (+inf, -inf, zeros) without a launch.  Refused on the host before anything is allocated or launched, with return
 * value 2: a NULL argument, n_dirs < 1 or > 2^20, a direction that is zero, not finite or not of unit length to 1e-12, sin_limit
 * outside [0, 1), bed_tol negative or NaN, 2^31 or more triangles.  Other failures return 1. */
int sdf_mesh_overhangs(sdf_mesh *mesh, const double *h_dirs, int64_t n_dirs, double sin_limit, double bed_tol, size_t max_scratch_bytes,
                       double *h_values, int64_t *h_counts);
int sdf_mesh_overhang_classes(sdf_mesh *mesh, const double *h_dir3, double sin_limit, double bed_tol, uint8_t *h_classes);
/* the kernels of this thread's last sdf_mesh_overhangs or sdf_mesh_overhang_classes alone, milliseconds by HIP events; *n_slabs (or
 * NULL): the slabs of directions that call took (tools/overhang_time.py) */
double sdf_overhang_last_kernel_ms(int64_t *n_slabs);
/* Support rays traced through the field: the true support volume of a build direction (added under ABI 17: the version is unchanged,
 * nothing above changes; DESIGN.md section 4o, defined by tests/supports_ref.py and reproduced bit for bit).  For the float64 soup of a
 * mesh in the field f of `tape` and n_dirs UNIT directions d, one after another: the faces are the triangles that
 * sdf_mesh_overhang_classes gives class 1 (overhang) for sin_limit and bed_tol, in triangle order, M of them; lo, hi are that rating's.
 * Per face: n and dn as there, proj = -dn (twice the area projected on the bed); the centroid c = ((a + b) + c) / 3.0 per coordinate;
 * tb = max(((cx dx + cy dy) + cz dz) - lo, 0), the distance to the bed plane.  A ray is sphere-traced from c along -d starting at
 * t = start: start >= tb ends it as BED (0) with height tb and no evaluation; otherwise at most max_steps times v = f(c + t (-d)): NaN
 * ends it as NAN (4, height NaN); v < 0 ends it with hi = t -- on the first evaluation as BURIED (2, height +0: the face has material
 * `start` below it), later as PART (1); otherwise lo = t and t advances by max(v * step_scale, min_step), and t >= tb ends it as BED
 * with height tb.  A ray that runs out of steps is UNRESOLVED (3) with height tb, an upper bound.  The bracket of a PART ray is bisected
 * `refine` times (the midpoint goes to hi where f < 0 there, else to lo) and its height is hi.  The five terms of a ray: proj * height
 * if BED or UNRESOLVED; proj * height if PART; proj if PART; proj; proj if BURIED -- else +0 -- summed over the M RAYS IN THEIR ORDER
 * through the tree of sdf_mesh_overhangs (chunks of 1024 consecutive rays, then groups of 256 halved).  s0 / 2 is the support volume
 * that stands on the bed, s1 / 2 the volume that stands on the part, s2 / 2 the projected area where supports touch the part, s3 / 2
 * the projected area of all overhangs, s4 / 2 that of the buried ones.  One ray per face is first-order quadrature; a gap narrower
 * than min_step can be stepped over; the columns are vertical.
 *   params8 = sin_limit, bed_tol, start, min_step, step_scale, 0, 0, 0 (reserved).
 *   h_values: n_dirs x 7 float64 (lo, hi, s0 .. s4); h_counts: n_dirs x 6 int64 (rays that ended BED, PART, BURIED, UNRESOLVED, NAN; M).
 *   sdf_support_rays_fetch copies the rays of direction k out -- h_triangle M int32, h_height M float64, h_status M uint8, h_steps M
 *   int32 (evaluations of the march), h_origin M x 3 float64; any pointer may be NULL -- and sdf_support_rays_destroy frees the handle
 *   and its device blocks (one per direction with rays, 41 bytes a ray).
 * Float64, the interpreter of sdf_eval_points.  It serves generated meshes, meshes of sdf_generate_records, adopted soups, selections,
 * simplified and mended meshes.  Synchronous, on the context's stream, one wait per direction (for M); one scratch allocation (49
 * bytes per triangle and the library scan's), sized once and freed before the call returns whether it fails or not.  A mesh of 0
 * triangles gives the empty result (+inf, -inf, zeros, M = 0) without a launch.  Refused on the host before anything is allocated or
 * launched, with return value 2: a NULL argument, a mesh without a soup on the device, a tape of another context, a tape with user
 * closures (sdf_tape_extern_count > 0), a non-finite parameter, start or min_step not above 0, step_scale outside (0, 1], sin_limit
 * outside [0, 1), bed_tol negative, max_steps < 1, refine < 0, n_dirs < 1 or > 1024, a direction that is zero, not finite or not of
 * unit length to 1e-12, 2^31 or more triangles; for the fetch a direction index out of range.  Other failures return 1, nothing stays
 * allocated and *out is NULL. */
typedef struct sdf_support_rays sdf_support_rays;
int sdf_mesh_support_rays(sdf_mesh *mesh, sdf_tape *tape, const double *h_dirs, int64_t n_dirs, const double *params8, int max_steps,
                          int refine, sdf_support_rays **out, double *h_values, int64_t *h_counts);
int sdf_support_rays_fetch(sdf_support_rays *rays, int64_t k, int32_t *h_triangle, double *h_height, uint8_t *h_status, int32_t *h_steps,
                           double *h_origin);
int sdf_support_rays_destroy(sdf_support_rays *rays);
/* the kernels of this thread's last sdf_mesh_support_rays, milliseconds by HIP events, summed over the directions; parts4 (or NULL):
 * classes and extents, numbering, rays, sums (tools/supports_time.py) */
double sdf_mesh_supports_last_kernel_ms(double *parts4);
/* Dual contouring of the field on a dense grid: a mesh with sharp creases (added under ABI 17: the version is unchanged, nothing
 * above changes; DESIGN.md section 4u, defined by tests/dual_ref.py and reproduced bit for bit).  Samples V[nx][ny][nz] at the axes'
 * points, s = (i * ny + j) * nz + k, inside iff v < 0.  The edge from sample s to its +1 neighbour along axis a is a crossing if
 * both ends are finite and differ in `inside`; crossings are numbered by ascending (s, a).  Its point: t = v0 / (v0 - v1),
 * p[a] = lo + t * (hi - lo); its normal: the field's, as sdf_mesh_vertex_normals takes it, step eps.  Every cell with a crossing
 * among its twelve edges is active and gets one vertex: over its crossings, in the order a = 0, 1, 2 and (db, dc) = (0, 0), (1, 0),
 * (0, 1), (1, 1) in the axes (a + 1) % 3, (a + 2) % 3, the mean m of q = p - centre and the quadric of the planes (n, n . q); the
 * system of sdf_mesh_simplify, (A + reg w I) y = b - A m with w the trace, x = m + y; w == 0: x = m (flat); a component that is
 * not finite: x = m (mean_fallback); else every component is clamped to the cell (clamped).  Active cells are numbered by ascending
 * index: the vertices.  Every crossing whose four cells exist emits two triangles over their vertices, (q0, q1, q2), (q0, q2, q3)
 * with the cells at (-1, -1), (0, -1), (0, 0), (-1, 0) in (b, c), reversed if the low end is not inside; a crossing on the grid's
 * border emits nothing (open_edges).
 *   *out            a mesh like sdf_mesh_simplify's: it owns its float64 soup and serves every reader; sdf_mesh_stats reports the
 *                   triangles and, with block > 0, the blocks of block^3 cells that hold / do not hold an active cell as n_nonempty /
 *                   n_empty (block <= 0: none are counted).
 *   h_counters8     crossings, cells, triangles, open_edges, nonfinite_edges (ends that differ in `inside`, one of them not finite:
 *                   no crossing), clamped, mean_fallback, flat.
 *   parts           NULL, or where to leave a handle to the crossing points and normals (crossings x 3 float64 each), the vertices
 *                   (cells x 3 float64) and the triangles' vertex indices (triangles x 3 int64): sdf_dual_parts_fetch copies them
 *                   out (any pointer may be NULL), sdf_dual_parts_destroy frees the handle's one device block.
 * Float64, the interpreter of sdf_eval_points over points made from the axes, in slabs of at most 2^22.  The grid is dense: 21 bytes
 * of device memory per sample (and the slab) in one scratch allocation, 61 per crossing in two more, 28 per vertex; all freed before
 * the call returns whether it fails or not.  Synchronous, on the context's stream.  An axis of fewer than 2 samples, or a grid
 * without a crossing, gives a mesh of 0 triangles.  Refused on the host before anything is allocated or launched, with return value
 * 2: a NULL pointer (parts aside), a tape of another context, a negative axis length, 2^31 or more samples, an eps that is not finite
 * and positive, a reg that is negative or not finite, an axis value that is not finite, a tape with user closures
 * (sdf_tape_extern_count > 0).  Other failures return 1 and *out is NULL. */
typedef struct sdf_dual_parts sdf_dual_parts;
int sdf_generate_dual(sdf_ctx *ctx, sdf_tape *tape, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, double eps,
                      double reg, int block, sdf_mesh **out, int64_t *h_counters8, sdf_dual_parts **parts);
int sdf_dual_parts_fetch(sdf_dual_parts *parts, double *h_points, double *h_normals, double *h_vertices, int64_t *h_cells);
int sdf_dual_parts_destroy(sdf_dual_parts *parts);
/* the kernels of this thread's last sdf_generate_dual, milliseconds by HIP events; parts5 (or NULL): the sampling, the crossings
 * (classify, scans, points), the normals, the cells and their vertices, the emission (tools/dual_time.py) */
double sdf_generate_dual_last_kernel_ms(double *parts5);
/* Pinned host memory for the results above: copies into it run at the link rate (fresh pageable memory:
 * ~10 GB/s).  Blocks are recycled through a small free list inside the library (pinning is slow), so
 * free what you allocate.  Any "host" pointer of this API may point into such a block. */
int sdf_host_alloc(size_t bytes, void **out);
int sdf_host_free(void *p);
/* per-batch classification, n_batches bytes: 0 skipped, 1 empty, 2 nonempty, 3 other shard */
int sdf_mesh_kinds(sdf_mesh *mesh, uint8_t *h_out);
/* diagnostics: what the interval prepass decided, 16 words per batch in batch order like
 * sdf_mesh_kinds (words 0..7: bit i set = instruction i skipped; 8..15: combine i takes its right
 * operand; decided for every batch, used by the ones that were meshed).  Fails when the mesh was
 * generated without the prepass. */
int sdf_mesh_prune_masks(sdf_mesh *mesh, uint32_t *h_out);
int sdf_mesh_destroy(sdf_mesh *mesh);

#ifdef __cplusplus
}
#endif
#endif /* SDF_HIP_H */
