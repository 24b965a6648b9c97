// sdf_prepass.hip -- what a generate call runs before k_mesh: the skip test of every batch (k_skip / k_skip_rare, the tape at nine
// points per batch; their surplus workgroups run the interval pruning pass of the same batches, sdf_prune.h), the pruning pass over the
// work list alone (k_prune_list) and the interval pass that decides which sampling tasks of a surviving batch are evaluated (k_cull /
// k_cull_lean / k_cull_lean128: cull_tasks, sdf_device.h) -- and the three host functions that launch them and nothing else:
// enqueue_skip, enqueue_prepass, enqueue_cull (declared in sdf_internal.h; the pipeline that calls them is sdf_generate.hip).
//
// Only k_skip and k_skip_rare run the tape; k_prune_list and the k_cull variants are INTERVAL interpreters that dispatch through a
// switch.  The unit takes the interpreters' flags, WITH the structurizer option (build.units), because k_skip needs it: its dispatch is
// the scalar jump through a table that the structurizer must leave alone.  Whether the interval kernels, whose lanes do diverge, are
// better off without the option has not been tried: with the prepass in a unit by itself that is this unit's line of build.units.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sdf_prune.h"
#include "sdf_plain.h"
#include "sdf_internal.h"

using namespace sdfk;

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
// meshing's scan and emission, the slab kernels, the STL records -- lives in sdf_plain.hip: see its head comment for why)

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

// ---- prepass: skip test for every batch, then the ordered work list (+ this shard's slice) ----
// interval pass: per batch, which instructions never matter.  tape_stride = 64-bit words per batch tape (0: no interval pass).
int enqueue_prepass(const GenCall &call, sdf_mesh *m, int nb, int tape_stride, hipStream_t st) {
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
int enqueue_cull(sdf_tape *t, sdf_mesh *m, int nb, int tape_stride, bool tail_order, int tail_max, hipStream_t st) {
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
