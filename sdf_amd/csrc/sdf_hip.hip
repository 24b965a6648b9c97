// sdf_hip.hip -- the tape-interpreter kernels (k_eval_*, k_skip, k_prune_list, k_cull) + the contexts, tapes and generate calls of
// libsdf_hip.so's C ABI (gfx950 only; the rest of the ABI: sdf_runtime.hip, sdf_chunked.hip, sdf_mesh_out.hip, sdf_comm.hip and the features' own units).  k_mesh is instantiated in sdf_mesh_inst.hip, k_estimate_bounds in sdf_bounds.hip, k_render in sdf_render.hip; every kernel that is not an
// interpreter (k_compact, k_scan_items, k_emit2, k_pack_slab, k_expand, k_mc_*, k_field_*, k_cast_f32, k_stl) in sdf_plain.hip.
//
// Kernels (one call of sdf_generate enqueues k_skip -> k_compact [-> k_prune_list] -> k_cull -> k_mesh
// [-> k_scan_items -> k_emit2] on one stream, without a host round trip in between)
//   k_eval_points / k_eval_grid   f(P): the tape interpreter alone; k_eval_points_ext: with user closures (L_EXTERN)
//   k_eval_tiles                  the float32 volumes of a chunk of batches of more than 33^3 samples (batch_size > 32: generate_big, sdf_chunked.hip)
//   k_estimate_bounds             the reference's `_estimate_bounds` loop (sdf/core.py:62-82) as one launch (sdf_bounds.hip)
//   k_skip                        the reference's `_skip` predicate for every batch at once
//                                 (reference sdf/core.py:28-43), 9 lanes per batch, 7 batches per wave; its surplus
//                                 workgroups run the interval pruning pass of the same batches (sdf_prune.h)
//   k_compact                     ordered work list of the surviving batches; clears the counters / look-back words
//   k_prune_list                  the pruning pass for the survivors only (grids with many batches)
//   k_cull / k_cull_lean          per surviving batch: the sampling tasks that have to be evaluated, by interval
//                                 arithmetic over groups of 4^3 cells (cull_tasks, sdf_device.h)
//   k_mesh (sdf_device.h)         THE hot kernel: one persistent workgroup per CU pulls batches
//                                 from the work list; samples the (<=33)^3 tile through the tape
//                                 interpreter (float64 -> float32 like skimage's cast) straight
//                                 into LDS (143,748 B of gfx950's 160 KiB), classifies the cells,
//                                 finds the batch's place in the ordered soup by a look-back over
//                                 the earlier batches' counts and writes the float64 world-space
//                                 triangles in reference order (reference `_worker`,
//                                 sdf/core.py:45-60, and `points.extend`, :141)
//   k_scan_items / k_emit2        two-pass meshing (long tapes): k_mesh stops at the classification, these number
//                                 and write the triangles
//   k_pack_slab / k_expand        multi-GPU exchange: a shard's soup as a fixed-capacity slab / the gathered slabs
//                                 expanded into the ordered float64 soup
//   k_mc_rows / k_mc_emit         marching cubes of a caller-supplied volume (`_marching_cubes`);
//   k_cast_f32 / k_field_*        the same for the chunks of batches that go through device memory (sdf_chunked.hip: a
//                                 host-evaluated field = user closures, and batch_size > 32)
//   k_stl                         50-byte STL records (reference sdf/stl.py:4-24)
//   k_vertex_normals              the field's gradient at the welded vertices (sdf_normals.hip); k_ply_vertices / k_ply_faces: binary PLY records
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mc_table.h"
#include "sdf_prune.h"
#include "sdf_plain.h"
#include "sdf_bounds.h"
#include "sdf_internal.h"

using namespace sdfk;

// ============================================================================================
// device side (the fused sample+march kernel k_mesh lives in sdf_device.h)
// ============================================================================================

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_eval_points(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                     const double *__restrict__ pts, long long n, int dim,
                                                     double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T x = (T)pts[i * dim], y = (T)pts[i * dim + 1], z = dim > 2 ? (T)pts[i * dim + 2] : T(0);
    out[i] = (double)run_tape1<T, FULL>(code, consts, x, y, z);
}

template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_eval_grid(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                   const double *__restrict__ X, const double *__restrict__ Y,
                                                   const double *__restrict__ Z, int nx, int ny, int nz,
                                                   double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = (long long)nx * ny * nz;
    if (i >= n) return;
    const int iz = (int)(i % nz), iy = (int)((i / nz) % ny), ix = (int)(i / ((long long)nz * ny));
    out[i] = (double)run_tape1<T, FULL>(code, consts, (T)X[ix], (T)Y[iy], (T)Z[iz]);
}

// `volume = sdf(P).reshape(...)`, cast to float32 as skimage does (reference sdf/core.py:50-54), for a chunk of whole tiles in
// device memory: batch_size > 32, whose (batch_size + 1)^3 tile does not fit the LDS of a compute unit (generate_big, sdf_chunked.hip).  One
// lane per sample; blockIdx.y = the tile (FieldTile: its place in `vol`, its extents), `org` its first sample per axis.
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_eval_tiles(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                    const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z,
                                                    const FieldTile *__restrict__ tiles, const int *__restrict__ org, float *__restrict__ vol) {
    const FieldTile tl = tiles[blockIdx.y];
    const long long n = (long long)tl.n0 * tl.n1 * tl.n2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int iz = (int)(i % tl.n2), iy = (int)((i / tl.n2) % tl.n1), ix = (int)(i / ((long long)tl.n2 * tl.n1));
    const int *o = org + 3 * blockIdx.y;
    vol[tl.vol_off + i] = (float)run_tape1<T, FULL>(code, consts, (T)X[o[0] + ix], (T)Y[o[1] + iy], (T)Z[o[2] + iz]);
}

// f(P) for tapes with user closures (L_EXTERN leaves): `dump` writes every leaf's current point for the host
// to call the closure on, the second pass reads the closures' values (sdf_interp.h ExtIO)
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_eval_points_ext(const uint32_t *__restrict__ code, const T *__restrict__ consts,
                                                         const double *__restrict__ pts, long long n, int dim,
                                                         double *__restrict__ ext, int dump, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T x = (T)pts[i * dim], y = (T)pts[i * dim + 1], z = dim > 2 ? (T)pts[i * dim + 2] : T(0);
    const T v = run_tape1_ext<T, FULL>(code, consts, x, y, z, ExtIO{ext, n, i, dump != 0});
    if (!dump) out[i] = (double)v;
}

// (k_estimate_bounds -- `_estimate_bounds`, reference sdf/core.py:62-82, as one launch -- lives in sdf_bounds.hip, built next to this unit)

// reference sdf/core.py:28-43.  9 lanes per batch, 7 batches per wave (lane 63 idles): lane 0 of a batch = centre,
// lanes 1..8 = corners in itertools.product((x0,x1),(y0,y1),(z0,z1)) order.  kinds[b] = 0 (skipped) or 255 (pending).
// (16 lanes per batch, 7 of them idle, until r02p: the kernel is the tape at 9 points per batch and nothing else.)
enum { SKIP_BATCHES_PER_BLOCK = 7 * (256 / 64) };
// Workgroups >= pa.first_block run the interval pass of the same batches instead (sdf_prune.h).
template <typename T, bool FULL, bool RARE>
__device__ __forceinline__ void skip_body(const uint32_t *__restrict__ code, const T *__restrict__ consts, GridDesc g,
                                              int nbatches, unsigned char *__restrict__ kinds, const PruneArgs &pa,
                                              const double *__restrict__ c64, const uint16_t *__restrict__ rstart,
                                              const uint16_t *__restrict__ lstart, double *prune_lds, int skip_b0) {
    if ((int)blockIdx.x >= pa.first_block) {   // (uniform)
        prune_block<FULL, RARE>(code, c64, rstart, lstart, pa, g, nbatches, (int)blockIdx.x - pa.first_block, prune_lds);
        return;
    }
    const int lane = threadIdx.x & 63, slot = min(lane / 9, 6), l = lane - 9 * slot;    // (lane 63: l = 9, idle)
    // (the skip test of batches [skip_b0, nbatches): a rank of a multi-GPU job tests its share only, sdf_skip_kinds)
    const int b = skip_b0 + ((int)blockIdx.x * (256 / 64) + (int)(threadIdx.x >> 6)) * 7 + slot;
    const bool live = b < nbatches && l < 9;
    int ox = 0, oy = 0, oz = 0, lx = 1, ly = 1, lz = 1;
    if (b < nbatches) batch_origin(g, b, ox, oy, oz, lx, ly, lz);
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
    if (b < nbatches) {
        x0 = g.X[ox]; x1 = g.X[ox + lx - 1]; y0 = g.Y[oy]; y1 = g.Y[oy + ly - 1]; z0 = g.Z[oz]; z1 = g.Z[oz + lz - 1];
    }
    const double cx = (x0 + x1) / 2, cy = (y0 + y1) / 2, cz = (z0 + z1) / 2;
    double px = cx, py = cy, pz = cz;
    if (l >= 1) { const int k = l - 1; px = (k & 4) ? x1 : x0; py = (k & 2) ? y1 : y0; pz = (k & 1) ? z1 : z0; }
    T v = T(0);
    if (live) v = run_tape1<T, FULL>(code, consts, (T)px, (T)py, (T)pz);
    const int base = 9 * slot;
    const T vc = __shfl(v, base, 64);          // centre
    const T v1 = __shfl(v, base + 1, 64);      // values[0]
    const bool pos = v1 > T(0);
    const bool ok = pos ? (v > T(0)) : (v < T(0));
    const unsigned long long m = __ballot(ok);
    const bool all_same = ((m >> (base + 1)) & 0xFFull) == 0xFFull;
    if (b < nbatches && l == 0) {
        const double r = fabs((double)vc);
        const double d = sqrt(((cx - x0) * (cx - x0) + (cy - y0) * (cy - y0)) + (cz - z0) * (cz - z0));
        const bool skip = !(r <= d) && all_same;
        kinds[b] = skip ? 0 : 255;
    }
}

// (two entry points: tapes with one of the less common leaves of ia_leaf_rare get the interval pass that knows
// them, the others keep the leaner one -- a kernel's registers and scratch are those of its hungriest callee)
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_skip(const uint32_t *__restrict__ code, const T *__restrict__ consts, GridDesc g,
                                              int nbatches, unsigned char *__restrict__ kinds, PruneArgs pa,
                                              const double *__restrict__ c64, const uint16_t *__restrict__ rstart, const uint16_t *__restrict__ lstart,
                                              int skip_b0) {
    extern __shared__ double prune_lds[];
    skip_body<T, FULL, false>(code, consts, g, nbatches, kinds, pa, c64, rstart, lstart, prune_lds, skip_b0);
}
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_skip_rare(const uint32_t *__restrict__ code, const T *__restrict__ consts, GridDesc g,
                                                   int nbatches, unsigned char *__restrict__ kinds, PruneArgs pa,
                                                   const double *__restrict__ c64, const uint16_t *__restrict__ rstart, const uint16_t *__restrict__ lstart,
                                                   int skip_b0) {
    extern __shared__ double prune_lds[];
    skip_body<T, FULL, true>(code, consts, g, nbatches, kinds, pa, c64, rstart, lstart, prune_lds, skip_b0);
}

// The interval pass of sdf_prune.h as a kernel of its own, over this shard's work list: for grids with many
// batches, most of which the skip test removes (weave at 2^33: 266 k batches, 38 k survive), pruning only the
// survivors is worth the extra launch behind k_compact; small grids keep it fused into k_skip's launch, where
// it costs nothing on the critical path.
template <bool FULL, bool RARE>
__global__ __launch_bounds__(PRUNE_BLOCK) void k_prune_list(const uint32_t *__restrict__ code, GridDesc g, int nbatches, PruneArgs pa,
                                                               const double *__restrict__ c64, const uint16_t *__restrict__ rstart,
                                                               const uint16_t *__restrict__ lstart) {
    extern __shared__ double prune_list_lds[];
    if ((long long)blockIdx.x * (PRUNE_BLOCK / 8) >= (long long)(pa.ctr->work_end - pa.ctr->work_begin)) return;   // (uniform)
    prune_block<FULL, RARE>(code, c64, rstart, lstart, pa, g, nbatches, (int)blockIdx.x, prune_list_lds);
}

// One workgroup per work item of this shard: which sampling tasks of the batch have to be evaluated
// (cull_tasks, sdf_device.h).  The record goes to global memory; k_mesh picks it up.
#define CULL_BLOCK 256
template <bool FULL, bool RARE, int CB = CULL_BLOCK>
__device__ __forceinline__ void cull_body(const uint32_t *__restrict__ code, const double *__restrict__ consts, GridDesc g,
                                                     const int *__restrict__ worklist, const MeshCounters *__restrict__ ctr,
                                                     int tape_stride, int n_instr, int ia_np, int ia_nd, int ia_bytes,
                                                     unsigned char *__restrict__ out, unsigned char *cull_smem, unsigned long long *prof,
                                                     int *__restrict__ order, int tail_max, int levels) {
    int *wave_sums = reinterpret_cast<int *>(cull_smem);                       // 64 B
    double *axes = reinterpret_cast<double *>(cull_smem + 64);                 // 3 * 33 doubles
    unsigned char *scratch = cull_smem + 896;                                  // CULL_SCRATCH bytes
    double *ia_state = reinterpret_cast<double *>(cull_smem + 896 + CULL_SCRATCH);
    const int tid = threadIdx.x;
    const long long tstart = prof ? clock64() : 0;
    // (one workgroup per BATCH is launched -- the host does not know the length of the work list -- and the surplus ones
    // leave here.  Striding over the list with a grid sized for the compute units was measured in r02: the loop costs the
    // kernel 10 - 20 % (example 60 -> 70 us, gearlike 2^30 prepass 0.36 -> 0.43 ms), the empty workgroups nothing.)
    // (the grid's pointers and sizes out of the kernel-argument segment NOW, next to the counters' load: the compiler
    // fetches a by-value struct's fields where they are first used, i.e. one dependent scalar-memory trip at a time)
    asm volatile("" :: "s"(g.X), "s"(g.Y), "s"(g.Z), "s"(g.nx), "s"(g.ny), "s"(g.nz), "s"(g.nby), "s"(g.nbz), "s"(g.bs));
    const int w = ctr->work_begin + (int)blockIdx.x;
    if (w >= ctr->work_end) return;
    long long t_ctr = 0, t_b = 0;
    if (prof) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_ctr) : "s"(w) : "memory");
    const int b = __builtin_amdgcn_readfirstlane(worklist[w]);   // (uniform: the tape is then read with scalar loads)
    if (prof) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_b) : "s"(b) : "memory");
    int ox, oy, oz, lx, ly, lz;
    batch_origin(g, b, ox, oy, oz, lx, ly, lz);
    long long t_org = 0;
    if (prof) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_org) : "s"(ox), "s"(oy), "s"(oz), "s"(lx) : "memory");
    for (int i = tid; i < 99; i += CB) {   // (ONE load per lane whatever the axis: three branches were three loads in a row for the first wave)
        const int ax = i < 33 ? 0 : (i < 66 ? 1 : 2), k = i - 33 * ax;
        const double *src = ax == 0 ? g.X + ox : (ax == 1 ? g.Y + oy : g.Z + oz);
        if (k < (ax == 0 ? lx : (ax == 1 ? ly : lz))) axes[i] = src[k];
    }
    long long t_ax = 0, t_bar = 0;
    if (prof) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_ax) : "s"(b) : "memory");
    __syncthreads();
    if (prof) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_bar) : "s"(b) : "memory");
    const uint32_t *wcode = code + (size_t)b * (size_t)tape_stride * 2;
    const int n_instr_w = tape_stride ? (int)reinterpret_cast<const unsigned long long *>(wcode)[tape_stride - 1] : n_instr;
    long long tstart1 = 0;   // (profiling: the clock once the work item, its axes and the length of its tape have arrived)
    if (prof) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tstart1) : "s"(n_instr_w) : "memory");
    const int ntl = cull_tasks<CB, FULL, RARE>(wcode, consts, n_instr_w, lx, ly, lz, axes, ia_state, ia_bytes, scratch, wave_sums, ia_np, ia_nd, prof, levels);
    const long long tw = prof ? clock64() : 0;
    if (tid == 0 && ntl < 0) reinterpret_cast<unsigned short *>(scratch)[0] = (unsigned short)0xFFFF;   // (else: the number of listed units, cull_tasks)
    __syncthreads();
    {   // the record: header + the listed units (whole tasks), and the sub-group states
        unsigned *rec = reinterpret_cast<unsigned *>(out + (size_t)w * CULL_RECORD);
        const unsigned *src = reinterpret_cast<const unsigned *>(scratch);
        const int nwords = ntl < 0 ? 1 : (CULL_ULIST + 16 * ntl + 3) >> 2;
        for (int i = tid; i < nwords; i += CB) rec[i] = src[i];
        if (ntl >= 0) for (int i = tid; i < (CULL_RECORD - CULL_SSTATE) / 4; i += CB) rec[CULL_SSTATE / 4 + i] = src[CULL_SSTATE / 4 + i];   // sub-group states + column words
    }
    // ---- every work item of the tail of the list leaves its cost estimate for k_mesh, which hands the tail out by
    // descending cost (MeshArgs::order) ----
    if (order && tid == 0) {
        const int tail = min(tail_max, ctr->work_end - ctr->work_begin), tpos = w - (ctr->work_end - tail);
        if (tpos >= 0) order[tpos] = (ntl < 0 ? 563 : ntl) * max(n_instr_w, 1);
    }
    if (prof && tid == 0) {
        const unsigned *pacc = reinterpret_cast<const unsigned *>(scratch + CULL_PACC);
        atomicAdd(&prof[32 + (ntl < 0 ? 9 : min(ntl >> 6, 8))], 1ull);   // histogram of the listed tasks per work item, bins of 64
        atomicAdd(&prof[16], (unsigned long long)(tstart1 - tstart));
        atomicAdd(&prof[26], (unsigned long long)(t_ctr - tstart));      // ... of which: until the shard's range is known
        atomicAdd(&prof[27], (unsigned long long)(t_b - t_ctr));         // ... until the batch index is
        atomicAdd(&prof[28], (unsigned long long)(t_ax - t_org));        // ... until this wave's axis values are in LDS
        atomicAdd(&prof[30], (unsigned long long)(t_org - t_b));         // ... (before that: the batch's origin from its index)
        atomicAdd(&prof[29], (unsigned long long)(t_bar - t_ax));        // ... its wait at the barrier (the workgroup's other waves)
        atomicAdd(&prof[21], (unsigned long long)(clock64() - tw));
        for (int k = 1; k < 10; k++) if (k != 5) atomicAdd(&prof[16 + k], (unsigned long long)pacc[k]);
    }
}

template <bool FULL, bool RARE, int CB = CULL_BLOCK>
__global__ __launch_bounds__(CB) void k_cull(const uint32_t *__restrict__ code, const double *__restrict__ consts, GridDesc g,
                                                     const int *__restrict__ worklist, const MeshCounters *__restrict__ ctr,
                                                     int tape_stride, int n_instr, int ia_np, int ia_nd, int ia_bytes,
                                                     unsigned char *__restrict__ out, unsigned long long *prof,
                                                     int *__restrict__ order, int tail_max, int levels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cull_smem[];
    cull_body<FULL, RARE, CB>(code, consts, g, worklist, ctr, tape_stride, n_instr, ia_np, ia_nd, ia_bytes, out, cull_smem, prof, order, tail_max, levels);
}
// the variant for tapes without trigonometry and without the rarer leaves: 70 VGPRs without spilling, seven waves per
// SIMD (the others take 99 - 104; holding them to five or six waves was measured in r02p: no faster)
__global__ __launch_bounds__(CULL_BLOCK) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_cull_lean(const uint32_t *__restrict__ code, const double *__restrict__ consts, GridDesc g,
                                                     const int *__restrict__ worklist, const MeshCounters *__restrict__ ctr,
                                                     int tape_stride, int n_instr, int ia_np, int ia_nd, int ia_bytes,
                                                     unsigned char *__restrict__ out, unsigned long long *prof,
                                                     int *__restrict__ order, int tail_max, int levels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cull_smem[];
    cull_body<false, false>(code, consts, g, worklist, ctr, tape_stride, n_instr, ia_np, ia_nd, ia_bytes, out, cull_smem, prof, order, tail_max, levels);
}
// (experiment: the same with two waves per workgroup -- twelve workgroups fit a CU, every work item of the 512^3
// example is resident at once instead of in two rounds)
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_cull_lean128(const uint32_t *__restrict__ code, const double *__restrict__ consts, GridDesc g,
                                                     const int *__restrict__ worklist, const MeshCounters *__restrict__ ctr,
                                                     int tape_stride, int n_instr, int ia_np, int ia_nd, int ia_bytes,
                                                     unsigned char *__restrict__ out, unsigned long long *prof,
                                                     int *__restrict__ order, int tail_max, int levels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cull_smem[];
    cull_body<false, false, 128>(code, consts, g, worklist, ctr, tape_stride, n_instr, ia_np, ia_nd, ia_bytes, out, cull_smem, prof, order, tail_max, levels);
}

// (every kernel that is not a tape interpreter -- the compaction, marching cubes of caller-supplied volumes, the two-pass
// meshing's scan and emission, the slab kernels, the STL records -- lives in sdf_plain.hip: see build.sh for why)

// ============================================================================================
// host side: contexts, tapes and the generate pipeline (the runtime underneath: sdf_runtime.h; the handles: sdf_internal.h; what
// reads a finished mesh: sdf_mesh_out.hip; the multi-GPU step: sdf_comm.hip; each further feature its own unit)
// ============================================================================================

static bool tape_needs_full(const uint32_t *code, uint32_t n_words, const double *consts) {
    auto trig_ease = [](int id) {
        return id == EASE_in_sine || id == EASE_out_sine || id == EASE_in_out_sine || id == EASE_in_expo ||
               id == EASE_out_expo || id == EASE_in_out_expo || id == EASE_in_elastic || id == EASE_out_elastic ||
               id == EASE_in_out_elastic;
    };
    for (uint32_t i = 0; i + 1 < n_words; i += 2) {
        const uint32_t op = code[i] & 255u;
        const double *c = consts + (code[i + 1] & 0xFFFFFFu) + 1;
        switch (op) {
        case OP_TWIST: case OP_BEND: case OP_BEND_RADIAL: case OP_WRAP_AROUND: case OP_CIRC_PREP: case OP_CIRC_SET:
        case OP_TRANS_RAD_PRE:
            return true;
        case OP_BEND_LINEAR: if (trig_ease((int)c[10])) return true; break;
        case OP_TRANS_LIN_PRE: if (trig_ease((int)c[7])) return true; break;
        case OP_EXTTO_PRE: if (trig_ease((int)c[1])) return true; break;
        default: break;
        }
    }
    return false;
}

static int validate_tape(const uint32_t *code, uint32_t n_words, uint32_t n_consts, uint32_t n_p, uint32_t n_d) {
    if (n_words < 2 || (n_words & 1)) return fail("tape: code must be a non-empty list of 2-word instructions");
    if (n_p > SDF_NP_SLOTS || n_d > SDF_ND_SLOTS) return fail("tape: model needs more register slots than this build provides");
    if ((code[n_words - 2] & 255u) != OP_END) return fail("tape: missing END");
    for (uint32_t i = 0; i < n_words; i += 2) {
        const uint32_t w0 = code[i], w1 = code[i + 1], op = w0 & 255u, post = (w0 >> 8) & 7u, sa = w0 >> 24, sb = w1 >> 24;
        if (op >= OP_COUNT) return fail("tape: unknown opcode");
        if (post > POST_BLEND) return fail("tape: unknown post-combine");
        if (w0 & 0x800000u) return fail("tape: reserved bit set");
        if ((w0 & 0x000800u) && ((w0 >> 12) & 7u) >= std::max(n_p, 1u)) return fail("tape: reload slot out of range");
        if ((w0 & 0x008000u) && ((w0 >> 16) & 7u) >= std::max(n_p, 1u)) return fail("tape: save slot out of range");
        if ((w0 & 0x080000u) && ((w0 >> 20) & 7u) >= std::max(n_d, 1u)) return fail("tape: push slot out of range");
        if (sa >= SDF_NP_SLOTS || sb >= SDF_NP_SLOTS) return fail("tape: slot out of range");
        if ((w1 & 0xFFFFFFu) >= n_consts) return fail("tape: constant offset out of range");
        if (op == OP_END && i != n_words - 2) return fail("tape: END before the last instruction");
    }
    return 0;
}

static int ctx_init(sdf_ctx *c);

extern "C" {

int sdf_abi_version(void) { return SDF_ABI_VERSION; }

#ifndef SDF_BUILD_INFO
#define SDF_BUILD_INFO "unknown toolchain (not built by csrc/build.sh)"
#endif
const char *sdf_build_info(void) { return SDF_BUILD_INFO; }

int sdf_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return 0; }
    return n;
}


int sdf_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes) {
    if (!free_bytes || !total_bytes) return fail("sdf_device_mem_info: NULL argument");
    HIPCHK(set_device(device));
    HIPCHK(hipMemGetInfo(free_bytes, total_bytes));
    return 0;
}

int sdf_ctx_create(int device, sdf_ctx **out) {
    if (!out) return fail("sdf_ctx_create: out is NULL");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail("sdf_ctx_create: no such device");
    HIPCHK(set_device(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(std::string("sdf_ctx_create: this library is built for gfx950 only, device is ") + prop.gcnArchName);
    sdf_ctx *c = new sdf_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    c->lds_max = prop.sharedMemPerBlock;
    if (ctx_init(c)) {          // (whatever was created so far goes back)
        const std::string keep = g_err;
        sdf_ctx_destroy(c);
        g_err = keep;
        return 1;
    }
    *out = c;
    return 0;
}

static int ctx_init(sdf_ctx *c) {
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    for (auto &e : c->ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(host_malloc(&c->h_stage, (size_t)SDF_CALL_SLOTS * SDF_STAGE_BYTES + 4096));   // (+ the bounds estimate's result, sdf_estimate_bounds)
    for (auto &cs : c->slots) {
        HIPCHK(hipEventCreate(&cs.e0)); HIPCHK(hipEventCreate(&cs.e2)); HIPCHK(hipEventCreate(&cs.e3)); HIPCHK(hipEventCreate(&cs.e4));
        HIPCHK(hipEventCreateWithFlags(&cs.done, hipEventDisableTiming));
        HIPCHK(hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking));
    }
    if (const char *e = getenv("SDF_SLOT_STREAMS")) c->slot_streams = atoi(e);
    if (const char *e = getenv("SDF_CULL_BLOCK")) c->cull_block = atoi(e);
    if (const char *e = getenv("SDF_TAIL_ORDER")) c->tail_order = atoi(e);
    if (const char *e = getenv("SDF_MESH_TWOPASS")) c->twopass = atoi(e);
    McTables t;
    memcpy(t.ntri, MC_NTRI, 256);
    memcpy(t.amb, MC_AMBIGUOUS, 256);
    memcpy(t.tri, MC_TRI, sizeof(t.tri));
    memcpy(t.mc33, MC33_FLAT, sizeof(t.mc33));
    if (c->mc.ensure(sizeof(t))) return 1;
    HIPCHK(hipMemcpy(c->mc.p, &t, sizeof(t), hipMemcpyHostToDevice));
    if (const char *e = getenv("SDF_BOUNDS_TAG0")) c->bounds_tag0 = (unsigned)atoi(e) & 0xFFFFu;   // (tests: the first tag of the exchange words)
    if (const char *e = getenv("SDF_MESH_SLOTS")) c->mesh_slots = atoi(e);
    if (const char *e = getenv("SDF_PRUNE")) c->prune = atoi(e);
    if (const char *e = getenv("SDF_PARK")) c->parking = atoi(e);
    if (const char *e = getenv("SDF_PRUNE_LIST_MIN")) c->prune_list_min = std::max(atoi(e), 0);
    if (const char *e = getenv("SDF_CULL")) c->cull = atoi(e);
    if (const char *e = getenv("SDF_DEFER")) c->defer = atoi(e) ? 1 : 0;
    if (const char *e = getenv("SDF_CULL_LEVELS")) c->cull_levels = atoi(e);
    if (const char *e = getenv("SDF_PARK_SPINS")) c->park_spins = std::max(atoi(e), 1);
    if (const char *e = getenv("SDF_MESH_PROF")) { if (atoi(e) && c->prof.ensure(512 + 4096 * 32)) return 1; }
    return 0;
}

int sdf_ctx_destroy(sdf_ctx *c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)stream_wait(c->stream);
    for (auto &cs : c->slots) { if (cs.stream) (void)stream_wait(cs.stream); cs.park.release(); }
    for (DevBuf *b : {&c->scratch_in, &c->scratch_out, &c->rows, &c->rows_off, &c->mc, &c->prof, &c->park, &c->ext, &c->field_vals,
                      &c->field_vol, &c->field_tiles, &c->bounds_work})
        b->release();
    for (auto &b : c->arena_pool) b.release();
    for (auto &b : c->counter_pool) b.release();
    g_pool.drop_device(c->device);
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto &cs : c->slots) for (hipEvent_t e : {cs.e0, cs.e2, cs.e3, cs.e4, cs.done}) if (e) (void)hipEventDestroy(e);
    for (auto &cs : c->slots) if (cs.stream) (void)hipStreamDestroy(cs.stream);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_rec) (void)hipHostFree(c->h_rec);
    for (hipEvent_t e : c->rec_ev) if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return 0;
}

int sdf_ctx_set_stream(sdf_ctx *c, void *s) {
    if (!c) return fail("sdf_ctx_set_stream: ctx is NULL");
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return 0;
}

int sdf_ctx_set_prune(sdf_ctx *c, int enabled) {
    if (!c) return fail("sdf_ctx_set_prune: ctx is NULL");
    c->prune = enabled ? 1 : 0;
    return 0;
}

int sdf_ctx_set_cull(sdf_ctx *c, int enabled) {
    if (!c) return fail("sdf_ctx_set_cull: ctx is NULL");
    c->cull = enabled ? 1 : 0;
    return 0;
}

int sdf_ctx_set_defer(sdf_ctx *c, int on) {
    if (!c) return fail("sdf_ctx_set_defer: ctx is NULL");
    c->defer = on ? 1 : 0;
    return 0;
}
int sdf_ctx_set_cull_levels(sdf_ctx *c, int levels) {
    if (!c) return fail("sdf_ctx_set_cull_levels: ctx is NULL");
    if (levels != 0 && levels != 2 && levels != 3) return fail("sdf_ctx_set_cull_levels: 0 (the library's choice), 2 or 3");
    c->cull_levels = levels;
    return 0;
}

int sdf_ctx_set_tail_order(sdf_ctx *c, int on) {
    if (!c) return fail("sdf_ctx_set_tail_order: ctx is NULL");
    c->tail_order = on ? 1 : 0;
    return 0;
}
int sdf_ctx_set_twopass(sdf_ctx *c, int mode) {
    if (!c) return fail("sdf_ctx_set_twopass: ctx is NULL");
    c->twopass = mode < 0 ? -1 : (mode ? 1 : 0);
    return 0;
}

// hand the device memory the library keeps for reuse (blocks of destroyed meshes, soup and counter pools) back to the
// driver: for a caller that switches to a job of a very different size -- the cached blocks of the old job do not fit the
// new one and would be evicted one by one, each hipFree a device synchronisation in the middle of the new job's calls
int sdf_ctx_trim(sdf_ctx *c) {
    if (!c) return fail("sdf_ctx_trim: ctx is NULL");
    HIPCHK(set_device(c->device));
    HIPCHK(stream_wait(c->stream));
    for (auto &cs : c->slots) if (cs.stream) HIPCHK(stream_wait(cs.stream));
    for (auto &b : c->arena_pool) b.release();
    c->arena_pool.clear();
    g_pool.drop_device(c->device);
    return 0;
}

int sdf_ctx_synchronize(sdf_ctx *c) {
    if (!c) return fail("sdf_ctx_synchronize: ctx is NULL");
    HIPCHK(set_device(c->device));
    HIPCHK(stream_wait(c->stream));
    for (auto &cs : c->slots) if (cs.stream) HIPCHK(stream_wait(cs.stream));
    return 0;
}

int sdf_tape_create(sdf_ctx *c, const uint32_t *code, uint32_t n_words, const double *consts, uint32_t n_consts,
                    uint32_t n_p, uint32_t n_d, sdf_tape **out) {
    if (!c || !code || !consts || !out) return fail("sdf_tape_create: NULL argument");
    if (validate_tape(code, n_words, n_consts, n_p, n_d)) return 1;
    HIPCHK(set_device(c->device));
    sdf_tape *t = new sdf_tape();
    struct Guard { sdf_tape *t; ~Guard() { if (t) { const std::string keep = g_err; sdf_tape_destroy(t); g_err = keep; } } } guard{t};
    t->ctx = c; t->n_words = n_words; t->n_consts = n_consts;
    t->full = tape_needs_full(code, n_words, consts);
    {
        unsigned long long h = 1469598103934665603ull;
        auto mix = [&](const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
        mix(code, (size_t)n_words * 4); mix(consts, (size_t)n_consts * 8); mix(&n_p, 4); mix(&n_d, 4);
        t->content_hash = h;
    }
    t->ia_complete = true;
    for (uint32_t i = 0; i < n_words; i += 2) {
        t->ia_complete = t->ia_complete && ia_has_form(code[i] & 255u);
        t->ia_rare = t->ia_rare || ia_is_rare_leaf(code[i] & 255u);
        if ((code[i] & 255u) == OP_L_EXTERN) {
            if ((code[i + 1] & 0xFFFFFFu) + 1 >= n_consts) return fail("tape: closure index out of the constant pool");
            const double k = consts[(code[i + 1] & 0xFFFFFFu) + 1];
            if (!(k >= 0.0 && k < 65536.0 && k == (double)(uint32_t)k)) return fail("tape: bad closure index");
            t->n_extern = std::max(t->n_extern, (uint32_t)k + 1u);
        }
    }
    t->n_p = n_p; t->n_d = n_d;
    // two more constants behind the tape's own: a K slot and +0.0, the operand of the `acc + (+0.0)` that a
    // decided smooth combine turns into (sdf_interval.h compact_tape); an instruction with constant
    // offset n_consts reads it as c[0]
    std::vector<double> c64(consts, consts + n_consts);
    c64.push_back(0.0); c64.push_back(0.0);
    std::vector<float> c32(c64.size());
    for (size_t i = 0; i < c64.size(); i++) c32[i] = (float)c64[i];
    std::vector<uint32_t> pcode(code, code + n_words);   // + one more END: the interpreter looks one instruction ahead
    pcode.push_back(code[n_words - 2]); pcode.push_back(code[n_words - 1]);
    HIPCHK(dev_malloc((void **)&t->d_code, pcode.size() * sizeof(uint32_t)));
    HIPCHK(dev_malloc((void **)&t->d_c64, c64.size() * sizeof(double)));
    HIPCHK(dev_malloc((void **)&t->d_c32, c32.size() * sizeof(float)));
    HIPCHK(hipMemcpy(t->d_code, pcode.data(), pcode.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->d_c64, c64.data(), c64.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->d_c32, c32.data(), c32.size() * sizeof(float), hipMemcpyHostToDevice));
    guard.t = nullptr;
    *out = t;
    return 0;
}

int sdf_tape_set_prune_info(sdf_tape *t, const uint16_t *rstart, const uint16_t *lstart, uint32_t n_instr) {
    if (!t || !rstart || !lstart) return fail("sdf_tape_set_prune_info: NULL argument");
    if (n_instr * 2 != t->n_words) return fail("sdf_tape_set_prune_info: one entry per instruction expected");
    for (uint32_t i = 0; i < n_instr; i++) {
        const bool none = rstart[i] == 0xFFFF || lstart[i] == 0xFFFF;
        if (!none && !(lstart[i] <= rstart[i] && rstart[i] <= i)) return fail("sdf_tape_set_prune_info: operand range out of order");
    }
    HIPCHK(set_device(t->ctx->device));
    if (!t->d_rstart) HIPCHK(dev_malloc((void **)&t->d_rstart, n_instr * 2));
    if (!t->d_lstart) HIPCHK(dev_malloc((void **)&t->d_lstart, n_instr * 2));
    HIPCHK(hipMemcpy(t->d_rstart, rstart, n_instr * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->d_lstart, lstart, n_instr * 2, hipMemcpyHostToDevice));
    return 0;
}

int sdf_tape_destroy(sdf_tape *t) {
    if (!t) return 0;
    (void)hipSetDevice(t->ctx->device);
    // kernels that read the tape may still run on the context's stream, on a call slot's lane or on a communicator's lanes:
    // wait for the DEVICE (a tape is destroyed once per model, not per call)
    (void)hipDeviceSynchronize();
    if (t->d_code) (void)hipFree(t->d_code);
    if (t->d_c64) (void)hipFree(t->d_c64);
    if (t->d_c32) (void)hipFree(t->d_c32);
    if (t->d_rstart) (void)hipFree(t->d_rstart);
    if (t->d_lstart) (void)hipFree(t->d_lstart);
    delete t;
    return 0;
}

}  // extern "C"

// dispatch over (precision, FULL)
#define LAUNCH_TAPE(KERNEL, grid, block, shmem, t, precision, ...) \
    LAUNCH_TAPE_ON((t)->ctx->stream, KERNEL, grid, block, shmem, t, precision, __VA_ARGS__)   /* on the context's stream */

#define LAUNCH_TAPE_ON(STREAM, KERNEL, grid, block, shmem, t, precision, ...)                                   \
    do {                                                                                                        \
        if ((precision) == SDF_PRECISION_F64) {                                                                 \
            if ((t)->full) hipLaunchKernelGGL((KERNEL<double, true>), grid, block, shmem, STREAM, (t)->d_code, (t)->d_c64, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<double, false>), grid, block, shmem, STREAM, (t)->d_code, (t)->d_c64, __VA_ARGS__); \
        } else {                                                                                                \
            if ((t)->full) hipLaunchKernelGGL((KERNEL<float, true>), grid, block, shmem, STREAM, (t)->d_code, (t)->d_c32, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<float, false>), grid, block, shmem, STREAM, (t)->d_code, (t)->d_c32, __VA_ARGS__); \
        }                                                                                                       \
    } while (0)

extern "C" {

int sdf_eval_points(sdf_tape *t, const void *d_pts, int64_t n, int dim, void *d_out, int precision) {
    if (!t || !d_pts || !d_out) return fail("sdf_eval_points: NULL argument");
    if (dim != 2 && dim != 3) return fail("sdf_eval_points: dim must be 2 or 3");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_eval_points: bad precision");
    if (t->n_extern) return fail("sdf_eval_points: the tape reads user closures (L_EXTERN): use sdf_eval_extern_points_host / sdf_eval_points_extern_host");
    if (n <= 0) return 0;
    HIPCHK(set_device(t->ctx->device));
    const unsigned grid = (unsigned)((n + 255) / 256);
    LAUNCH_TAPE(k_eval_points, dim3(grid), dim3(256), 0, t, precision, (const double *)d_pts, (long long)n, dim, (double *)d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int sdf_eval_points_host(sdf_tape *t, const double *h_pts, int64_t n, int dim, double *h_out, int precision) {
    if (!t || !h_pts || !h_out) return fail("sdf_eval_points_host: NULL argument");
    if (dim != 2 && dim != 3) return fail("sdf_eval_points_host: dim must be 2 or 3");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_eval_points_host: bad precision");
    if (n <= 0) return 0;
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    if (c->scratch_in.ensure((size_t)n * dim * 8) || c->scratch_out.ensure((size_t)n * 8)) return 1;
    HIPCHK(hipMemcpyAsync(c->scratch_in.p, h_pts, (size_t)n * dim * 8, hipMemcpyHostToDevice, c->stream));
    if (sdf_eval_points(t, c->scratch_in.p, n, dim, c->scratch_out.p, precision)) return 1;
    HIPCHK(hipMemcpyAsync(h_out, c->scratch_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    return 0;
}

int sdf_eval_grid_host(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                       double *h_out, int precision) {
    if (!t || !X || !Y || !Z || !h_out) return fail("sdf_eval_grid_host: NULL argument");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_eval_grid_host: bad precision");
    if (t->n_extern) return fail("sdf_eval_grid_host: the tape reads user closures (L_EXTERN): evaluate it with the *_extern_* entry points");
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    const size_t n = (size_t)nx * ny * nz;
    if (c->scratch_in.ensure((size_t)(nx + ny + nz) * 8) || c->scratch_out.ensure(n * 8)) return 1;
    double *dX = (double *)c->scratch_in.p, *dY = dX + nx, *dZ = dY + ny;
    HIPCHK(hipMemcpyAsync(dX, X, (size_t)nx * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dY, Y, (size_t)ny * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dZ, Z, (size_t)nz * 8, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)((n + 255) / 256);
    LAUNCH_TAPE(k_eval_grid, dim3(grid), dim3(256), 0, t, precision, (const double *)dX, (const double *)dY, (const double *)dZ,
                nx, ny, nz, (double *)c->scratch_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, c->scratch_out.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    return 0;
}

int sdf_estimate_bounds(sdf_tape *t, double *h_out6, int precision) {
    if (!t || !h_out6) return fail("sdf_estimate_bounds: NULL argument");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_estimate_bounds: bad precision");
    if (t->n_extern) return fail("sdf_estimate_bounds: the tape reads user closures (L_EXTERN): probe it through the *_extern_* entry points");
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    if (c->scratch_out.ensure(4096)) return 1;
    // the waves' exchange words are tagged per call instead of zeroed per call (sdf_bounds.hip): cleared when the buffer is new and when
    // the 16-bit tag wraps
    if (!c->bounds_work.p || c->bounds_tag >= 65535u) {
        if (c->bounds_work.ensure(SDF_BOUNDS_WORK_BYTES)) return 1;
        HIPCHK(hipMemsetAsync(c->bounds_work.p, 0, SDF_BOUNDS_WORK_BYTES, c->stream));
        c->bounds_tag = c->bounds_tag0; c->bounds_tag0 = 0;
    }
    const unsigned tag = ++c->bounds_tag;
    {
        const int rc = sdf_launch_bounds(precision == SDF_PRECISION_F64 ? 1 : 0, t->full ? 1 : 0, c->stream, (const uint32_t *)t->d_code,
                                         precision == SDF_PRECISION_F64 ? (const void *)t->d_c64 : (const void *)t->d_c32, (double *)c->scratch_out.p,
                                         c->bounds_work.p, tag);
        if (rc) return fail(std::string("k_estimate_bounds launch: ") + hipGetErrorString((hipError_t)rc));
    }
    // (the seven doubles land in pinned memory behind the call slots' staging: a copy into pageable memory goes through the runtime's
    // own staging and a second host copy)
    double *h = (double *)((char *)c->h_stage + (size_t)SDF_CALL_SLOTS * SDF_STAGE_BYTES);
    HIPCHK(hipMemcpyAsync(h, c->scratch_out.p, 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    if (h[6] == 2.0) return fail("sdf_estimate_bounds: the probe workgroups did not meet at their barrier (device busy): use the host loop");
    if (h[6] != 0.0) return fail("zero-size array to reduction operation maximum which has no identity");   // (NumPy's words, reference sdf/core.py:80)
    memcpy(h_out6, h, 48);
    return 0;
}

int sdf_tape_extern_count(sdf_tape *t) { return t ? (int)t->n_extern : 0; }

// phase 1 of f(P) for a tape with user closures: the point every L_EXTERN leaf sees, per sample
int sdf_eval_extern_points_host(sdf_tape *t, const double *h_pts, int64_t n, int dim, double *h_ext_pts, int precision) {
    if (!t || !h_pts || !h_ext_pts) return fail("sdf_eval_extern_points_host: NULL argument");
    if (dim != 2 && dim != 3) return fail("sdf_eval_extern_points_host: dim must be 2 or 3");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_eval_extern_points_host: bad precision");
    if (!t->n_extern) return fail("sdf_eval_extern_points_host: the tape has no user closures");
    if (n <= 0) return 0;
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    const size_t ext_bytes = (size_t)t->n_extern * (size_t)n * 24;
    if (c->scratch_in.ensure((size_t)n * dim * 8) || c->ext.ensure(ext_bytes)) return 1;
    HIPCHK(hipMemcpyAsync(c->scratch_in.p, h_pts, (size_t)n * dim * 8, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)((n + 255) / 256);
    LAUNCH_TAPE(k_eval_points_ext, dim3(grid), dim3(256), 0, t, precision, (const double *)c->scratch_in.p, (long long)n, dim,
                (double *)c->ext.p, 1, (double *)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_ext_pts, c->ext.p, ext_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    return 0;
}

// phase 2: f(P) with the closures' values (n_extern x n float64, leaf-major) supplied by the host
int sdf_eval_points_extern_host(sdf_tape *t, const double *h_pts, int64_t n, int dim, const double *h_ext_vals, double *h_out,
                                int precision) {
    if (!t || !h_pts || !h_ext_vals || !h_out) return fail("sdf_eval_points_extern_host: NULL argument");
    if (dim != 2 && dim != 3) return fail("sdf_eval_points_extern_host: dim must be 2 or 3");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_eval_points_extern_host: bad precision");
    if (!t->n_extern) return fail("sdf_eval_points_extern_host: the tape has no user closures");
    if (n <= 0) return 0;
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    const size_t ext_bytes = (size_t)t->n_extern * (size_t)n * 8;
    if (c->scratch_in.ensure((size_t)n * dim * 8) || c->scratch_out.ensure((size_t)n * 8) || c->ext.ensure(ext_bytes)) return 1;
    HIPCHK(hipMemcpyAsync(c->scratch_in.p, h_pts, (size_t)n * dim * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->ext.p, h_ext_vals, ext_bytes, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)((n + 255) / 256);
    LAUNCH_TAPE(k_eval_points_ext, dim3(grid), dim3(256), 0, t, precision, (const double *)c->scratch_in.p, (long long)n, dim,
                (double *)c->ext.p, 0, (double *)c->scratch_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, c->scratch_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    return 0;
}

int sdf_marching_cubes(sdf_ctx *c, const void *d_volume, int n0, int n1, int n2, void *d_out, int64_t cap, int64_t *n_tris) {
    if (!c || !n_tris) return fail("sdf_marching_cubes: NULL argument");
    *n_tris = 0;
    if (n0 < 2 || n1 < 2 || n2 < 2) return 0;   // skimage: "Input array must be at least 2x2x2" -> empty batch
    if (!d_volume) return fail("sdf_marching_cubes: volume is NULL");
    HIPCHK(set_device(c->device));
    const long long nrows = (long long)(n0 - 1) * (n1 - 1);
    if (c->rows.ensure((size_t)nrows * 4) || c->rows_off.ensure((size_t)(nrows + 1) * 8)) return 1;
    unsigned long long *d_total = (unsigned long long *)c->rows_off.p + nrows;
    const unsigned grid = (unsigned)((nrows + 255) / 256);
    launch_k_mc_rows(dim3(grid), dim3(256), c->stream, (const McTables *)c->mc.p, (const float *)d_volume, n0, n1, n2, (unsigned *)c->rows.p);
    launch_k_scan_rows(dim3(1), dim3(1024), c->stream, (const unsigned *)c->rows.p, nrows,
                       (unsigned long long *)c->rows_off.p, d_total);
    HIPCHK(hipGetLastError());
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait(c->stream));
    *n_tris = (int64_t)total;
    if (total && d_out && cap > 0) {
        launch_k_mc_emit(dim3(grid), dim3(256), c->stream, (const McTables *)c->mc.p, (const float *)d_volume, n0, n1, n2,
                           (const unsigned long long *)c->rows_off.p, (float *)d_out, (unsigned long long)cap);
        HIPCHK(hipGetLastError());
        HIPCHK(stream_wait(c->stream));
    }
    return 0;
}

int sdf_marching_cubes_host(sdf_ctx *c, const float *h_vol, int n0, int n1, int n2, float *h_out, int64_t cap, int64_t *n_tris) {
    if (!c || !n_tris) return fail("sdf_marching_cubes_host: NULL argument");
    *n_tris = 0;
    if (n0 < 2 || n1 < 2 || n2 < 2) return 0;
    if (!h_vol) return fail("sdf_marching_cubes_host: volume is NULL");
    HIPCHK(set_device(c->device));
    const size_t n = (size_t)n0 * n1 * n2;
    if (c->scratch_in.ensure(n * 4)) return 1;
    if (cap > 0 && c->scratch_out.ensure((size_t)cap * 36)) return 1;
    HIPCHK(hipMemcpyAsync(c->scratch_in.p, h_vol, n * 4, hipMemcpyHostToDevice, c->stream));
    if (sdf_marching_cubes(c, c->scratch_in.p, n0, n1, n2, cap > 0 ? c->scratch_out.p : nullptr, cap, n_tris)) return 1;
    const int64_t ncopy = std::min<int64_t>(*n_tris, cap);
    if (ncopy > 0 && h_out) {
        HIPCHK(hipMemcpyAsync(h_out, c->scratch_out.p, (size_t)ncopy * 36, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(stream_wait(c->stream));
    }
    return 0;
}

}  // extern "C"

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
    const int rc = t->full ? sdf_launch_mesh_f64_full(slots, 0, a.twopass, grid, lds, st, (const uint32_t *)code, t->d_c64, a)
                           : sdf_launch_mesh_f64(slots, 0, a.twopass, grid, lds, st, (const uint32_t *)code, t->d_c64, a);
    if (rc) return fail(std::string("k_mesh launch: ") + hipGetErrorString((hipError_t)rc));
    return 0;
}

// the skip test (`_skip`, reference sdf/core.py:28-43) of batches [b0, b1) alone, enqueued on `st`: d_kinds[b] = 0 (skipped) or
// 255 (pending) for those batches; the axes are on the device already (X, then Y, then Z)
int enqueue_skip(sdf_tape *t, const double *d_axes, int nx, int ny, int nz, int bs, int b0, int b1, int precision,
                 unsigned char *d_kinds, hipStream_t st) {
    if (b1 <= b0) return 0;
    GridDesc g;
    grid_desc(nx, ny, nz, bs, g);
    g.X = d_axes; g.Y = d_axes + nx; g.Z = d_axes + nx + ny;
    PruneArgs pa = {};
    pa.first_block = 0x7fffffff;     // (no interval pass in this launch)
    const unsigned blocks = (unsigned)((b1 - b0 + SKIP_BATCHES_PER_BLOCK - 1) / SKIP_BATCHES_PER_BLOCK);
    LAUNCH_TAPE_ON(st, k_skip, dim3(blocks), dim3(256), 0, t, precision, g, b1, d_kinds, pa, (const double *)t->d_c64,
                   (const uint16_t *)t->d_rstart, (const uint16_t *)t->d_lstart, b0);
    HIPCHK(hipGetLastError());
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

// ---- prepass: skip test for every batch, then the ordered work list (+ this shard's slice) ----
// interval pass: per batch, which instructions never matter.  tape_stride = 64-bit words per batch tape (0: no interval pass).
static int enqueue_prepass(const GenCall &call, sdf_mesh *m, int nb, int tape_stride, hipStream_t st) {
    sdf_tape *t = call.tape;
    sdf_ctx *c = t->ctx;
    const GridDesc &g = m->g;
    const int sparse = call.sparse, precision = call.precision;
    const bool pruning = tape_stride != 0;
    const uint32_t n_instr = t->n_words / 2;
    PruneArgs pa = {};
    pa.first_block = 0x7fffffff;
    // many batches: the interval pass runs behind k_compact, for the surviving batches only (k_prune_list)
    // (a rank of a multi-GPU job prunes its own share of the work list only, whatever the grid's size)
    const bool prune_listed = pruning && sparse && (nb >= c->prune_list_min || call.shard_count > 1);
    unsigned skip_blocks = (sparse && !call.d_kinds) ? (unsigned)((nb + SKIP_BATCHES_PER_BLOCK - 1) / SKIP_BATCHES_PER_BLOCK) : 0u, prune_blocks = 0;
    size_t prune_lds = 0;
    if (pruning) {
        if (m->prune.ensure((size_t)nb * 64) || m->tapes.ensure((size_t)nb * tape_stride * 8)) return 1;
        pa.n_instr = (int)n_instr; pa.n_p = std::max(t->n_p, 1u); pa.n_d = std::max(t->n_d, 1u);
        pa.masks_out = (uint32_t *)m->prune.p; pa.tapes_out = (unsigned long long *)m->tapes.p; pa.tape_stride = tape_stride;
        pa.zero_off = t->n_consts;
        prune_lds = prune_lds_bytes(pa.n_p, pa.n_d);
        if (!prune_listed) {         // fused into k_skip's launch: every batch
            pa.first_block = (int)skip_blocks;
            prune_blocks = (unsigned)(((long long)nb * 8 + PRUNE_BLOCK - 1) / PRUNE_BLOCK);
        }
    }
    if (skip_blocks + prune_blocks) {
        if (prune_lds > 32768 && prune_blocks) {   // (more dynamic LDS than the default limit: tapes with many saved-point slots)
            const void *fn = t->ia_rare ? (t->full ? reinterpret_cast<const void *>(k_skip_rare<double, true>) : reinterpret_cast<const void *>(k_skip_rare<double, false>))
                                        : (t->full ? reinterpret_cast<const void *>(k_skip<double, true>) : reinterpret_cast<const void *>(k_skip<double, false>));
            HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)prune_lds));
        }
        const size_t skip_lds = prune_blocks ? prune_lds : 0;
        if (t->ia_rare) LAUNCH_TAPE_ON(st, k_skip_rare, dim3(skip_blocks + prune_blocks), dim3(256), skip_lds, t, precision, g, nb, (unsigned char *)m->kinds.p, pa,
                                       (const double *)t->d_c64, (const uint16_t *)t->d_rstart, (const uint16_t *)t->d_lstart, 0);
        else LAUNCH_TAPE_ON(st, k_skip, dim3(skip_blocks + prune_blocks), dim3(256), skip_lds, t, precision, g, nb, (unsigned char *)m->kinds.p, pa,
                            (const double *)t->d_c64, (const uint16_t *)t->d_rstart, (const uint16_t *)t->d_lstart, 0);
    }
    if (!sparse) HIPCHK(hipMemsetAsync(m->kinds.p, 255, (size_t)nb, st));
    else if (call.d_kinds) HIPCHK(hipMemcpyAsync(m->kinds.p, call.d_kinds, (size_t)nb, hipMemcpyDeviceToDevice, st));   // (k_mesh writes its verdicts into the mesh's own copy)
    launch_k_compact(dim3(1), dim3(1024), st, (const unsigned char *)m->kinds.p, nb, (int *)m->worklist.p,
                       (MeshCounters *)m->counters.p, (unsigned long long *)m->status.p, (long long)call.shard_index,
                       (long long)call.shard_count);
    HIPCHK(hipGetLastError());
    if (prune_listed) {
        pa.worklist = (const int *)m->worklist.p; pa.ctr = (const MeshCounters *)m->counters.p;
        auto kp = t->full ? (t->ia_rare ? k_prune_list<true, true> : k_prune_list<true, false>) : (t->ia_rare ? k_prune_list<false, true> : k_prune_list<false, false>);
        if (prune_lds > 32768) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)prune_lds));
        hipLaunchKernelGGL(kp, dim3((unsigned)(((long long)nb * 8 + PRUNE_BLOCK - 1) / PRUNE_BLOCK)), dim3(PRUNE_BLOCK), prune_lds, st,
                           (const uint32_t *)t->d_code, g, nb, pa, (const double *)t->d_c64, (const uint16_t *)t->d_rstart,
                           (const uint16_t *)t->d_lstart);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// second interval pass, per surviving batch: the sub-groups of 2^3 cells the surface cannot be in are not sampled.
// tail_order: every work item of the list's tail leaves its cost estimate in m->order.
static int enqueue_cull(sdf_tape *t, sdf_mesh *m, int nb, int tape_stride, bool tail_order, int tail_max, hipStream_t st) {
    sdf_ctx *c = t->ctx;
    const GridDesc &g = m->g;
    const bool pruning = tape_stride != 0;
    const uint32_t n_instr = t->n_words / 2;
    if (c->prof.p) HIPCHK(hipMemsetAsync((unsigned char *)c->prof.p + 128, 0, 384, st));
    if (m->cull.ensure((size_t)nb * CULL_RECORD) || (tail_order && m->order.ensure(MESH_TAIL_MAX * sizeof(int)))) return 1;
    const int ia_np = (int)std::max(t->n_p, 1u), ia_nd = (int)std::max(t->n_d, 1u);
    auto kc = t->full ? (t->ia_rare ? k_cull<true, true> : k_cull<true, false>) : (t->ia_rare ? k_cull<false, true> : k_cull_lean);
    int cull_block = CULL_BLOCK;
    if (c->cull_block == 128 && kc == k_cull_lean) { kc = k_cull_lean128; cull_block = 128; }
    // (the trig-capable variant with one or two waves per work item: the first level of the pass -- 64 boxes -- keeps
    // ONE wave of a workgroup busy whatever its size, so smaller workgroups mean more work items per compute unit)
    // measured (r03f, prepass of weave 2^33 / 2^27, gearlike 2^30, knurling 2^27, ms): 256 threads 8.95 / 1.52 / 0.325 /
    // 0.364; 128: 6.61 / 1.35 / 0.276 / 0.361; 64: 6.05 / 1.44 / 0.298 / 0.442 -- two waves are the default here
    if (t->full && !t->ia_rare && c->cull_block != 256) {
        cull_block = c->cull_block == 64 ? 64 : 128;
        kc = cull_block == 64 ? k_cull<true, false, 64> : k_cull<true, false, 128>;
    }
    // The third interval level (sub-groups of 2^3 cells) halves what k_mesh samples and costs 8 interval runs per
    // undecided group of 4^3 cells.  r04a, same box, prepass + k_mesh in ms, two levels -> three: example 2^27 0.068 + 0.280
    // -> 0.104 + 0.240, pawn 0.132 + 0.416 -> 0.276 + 0.289, blobby 2^30 0.229 + 0.874 -> 0.505 + 0.612 (level with or
    // ahead, and the prepass of the NEXT call hides behind k_mesh when calls are in flight); with trigonometry in the tape
    // the interval forms are dearer than the samples they save: gearlike 2^30 0.271 + 1.23 -> 0.64 + 0.99, knurling 2^27
    // 0.364 + 1.52 -> 1.58 + 1.25, weave 2^33 6.6 + 24.2 -> 19.9 + 15.4.  Hence three levels for the lean tapes, two for
    // the others -- which still list units of 2^3 samples instead of r03's cubes of 4^3.
    const int cull_levels = c->cull_levels ? c->cull_levels : (kc == k_cull_lean || kc == k_cull_lean128 ? 3 : 2);
    // (seven workgroups of 256 threads per CU instead of six -- 72 VGPRs, the interval state of 192 threads in LDS, so that
    // every work item of the 512^3 example is resident at once -- was measured in r04k: example prepass 0.093 vs 0.091 ms,
    // pawn 0.402 vs 0.266 ms: the levels then run in more passes.  Not the limit.)
    const size_t ia_bytes = std::min<size_t>((size_t)cull_block * (6 * ia_np + 2 * ia_nd) * 8, c->lds_max - 896 - CULL_SCRATCH);
    const size_t lds = 896 + CULL_SCRATCH + ia_bytes;
    if (lds > 32768) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kc, dim3(nb), dim3(cull_block), lds, st,
                       pruning ? (const uint32_t *)m->tapes.p : (const uint32_t *)t->d_code, (const double *)t->d_c64, g,
                       (const int *)m->worklist.p, (const MeshCounters *)m->counters.p, pruning ? tape_stride : 0, (int)n_instr,
                       ia_np, ia_nd, (int)ia_bytes, (unsigned char *)m->cull.p, (unsigned long long *)c->prof.p,
                       tail_order ? (int *)m->order.p : (int *)nullptr, tail_max, cull_levels);
    HIPCHK(hipGetLastError());
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
    const bool intervals_ok = call.precision == SDF_PRECISION_F64 && monotone(call.X, nx) && monotone(call.Y, ny) && monotone(call.Z, nz);
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

// k_eval_tiles for the nt tiles of a chunk (sdf_chunked.hip), the largest of largest_tile samples, enqueued on `st`: the axes, the
// tile table and the tiles' first samples `d_org` are on the device already; the caller checks the launch with the next ones
void enqueue_eval_tiles(sdf_tape *t, int precision, const double *dX, const double *dY, const double *dZ, const FieldTile *d_tiles,
                        const int *d_org, float *d_vol, size_t largest_tile, int nt, hipStream_t st) {
    LAUNCH_TAPE_ON(st, k_eval_tiles, dim3((unsigned)((largest_tile + 255) / 256), (unsigned)nt), dim3(256), 0, t, precision, dX, dY, dZ,
                   d_tiles, d_org, d_vol);
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
