// sdf_mend.hip -- a welded mesh mended on the device (sdf_mesh_mend, added under ABI 17): duplicate triangles
// are dropped and oppositely wound pairs cancel.  tests/mend_ref.py is the definition, and which triangles survive is a function of
// the welded cells alone: integers only, no floating point anywhere in this unit.
//
// A cell with two equal indices is collapsed.  Every other cell, rotated so that its smallest index a comes first, (a, b, c), has
// the FACE (a, min(b, c), max(b, c)) and the SIDE b > c: rotations agree in both, the flipped winding has the same face and the
// other side.  k_mend_keys: one lane per triangle writes two sort keys, lo = max << 1 | side (32 bits) and hi = a << vb | mid (vb =
// the bits that hold 0 .. V), and its own index as the value; a collapsed cell gets hi = V << vb, which sorts behind every live key,
// and is counted.  Two stable library sorts (hipCUB, like the weld's), least significant key first -- by lo carrying the index,
// k_mend_gather brings hi into that order, then by hi -- leave the triangles ordered by face, then side, then soup order.
//
// k_mend_runs: one lane per sorted position.  The lane whose face differs from its predecessor's is the head of a run; it walks the
// run, counts n0 and n1, and either sets the keep flag of the one survivor -- position head when side 0 has the majority, head + n0
// when side 1 has it: the first in soup order, because the sorts are stable -- or, n0 == n1, keeps nothing.  duplicates, cancelled
// and faces are summed across the workgroup and added with integer atomics, one per counter and workgroup (block_add of
// sdf_block.h).  A run is thousands of entries long only for a face repeated that often: legal, and slow for its lane only.
//
// Emission is a selection's: keep flags in soup order, number_flags, and the copy kernel of sdf_components.hip, nine doubles per
// survivor from the SOURCE soup, bit for bit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <string>

#include "sdf_block.h"
#include "sdf_components.h"
#include "sdf_mend.h"
#include "sdf_prims.h"

namespace sdfk {

// what the passes leave for the host
enum { DUPLICATES, CANCELLED, FACES, MEND_RUNS };                      // the counters of k_mend_runs, one block_add
struct MendHead {
    unsigned long long collapsed, runs[MEND_RUNS];
};

// one lane per triangle (n_tris, 3 n_tris and n_vertices are below 2^31: 32-bit indexing throughout)
__global__ __launch_bounds__(256) void k_mend_keys(const long long *__restrict__ cells, unsigned n_tris, unsigned n_vertices, int vb,
                                                   unsigned long long *__restrict__ hi, unsigned *__restrict__ lo, unsigned *__restrict__ idx,
                                                   MendHead *head) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    bool dead = false;
    if (t < n_tris) {
        const unsigned i0 = (unsigned)cells[3u * t], i1 = (unsigned)cells[3u * t + 1u], i2 = (unsigned)cells[3u * t + 2u];
        dead = i0 == i1 || i1 == i2 || i2 == i0;
        unsigned a = i2, b = i0, c = i1;
        if (i0 < i1 && i0 < i2) { a = i0; b = i1; c = i2; }
        else if (i1 < i0 && i1 < i2) { a = i1; b = i2; c = i0; }
        const unsigned side = b > c ? 1u : 0u, mid = side ? c : b, top = side ? b : c;
        hi[t] = dead ? (unsigned long long)n_vertices << vb : ((unsigned long long)a << vb) | mid;
        lo[t] = dead ? 0u : (top << 1) | side;
        idx[t] = t;
    }
    const bool is[1] = {dead};
    block_count(is, &head->collapsed);
}

// one lane per position of the order by lo
__global__ __launch_bounds__(256) void k_mend_gather(const unsigned long long *__restrict__ hi, const unsigned *__restrict__ idx, unsigned n_tris,
                                                     unsigned long long *__restrict__ hi_sorted) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p < n_tris) hi_sorted[p] = hi[idx[p]];
}

// one lane per position of the final order; hi, idx: in that order, lo: in soup order; dead_key: the hi of a collapsed cell; keep
// (soup order) was cleared beforehand
__global__ __launch_bounds__(256) void k_mend_runs(const unsigned long long *__restrict__ hi, const unsigned *__restrict__ idx,
                                                   const unsigned *__restrict__ lo, unsigned n_tris, unsigned long long dead_key,
                                                   int *__restrict__ keep, MendHead *head) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    unsigned duplicates = 0u, cancelled = 0u, faces = 0u;              // (the sums of one workgroup stay below the triangle count: 31 bits)
    if (p < n_tris) {
        const unsigned long long h = hi[p];
        if (h < dead_key) {
            const unsigned top = lo[idx[p]] >> 1;
            if (p == 0u || hi[p - 1u] != h || (lo[idx[p - 1u]] >> 1) != top) {
                unsigned n0 = 0u, n1 = 0u;
                for (unsigned q = p; q < n_tris && hi[q] == h; q++) {
                    const unsigned l = lo[idx[q]];
                    if ((l >> 1) != top) break;
                    if (l & 1u) n1 += 1u; else n0 += 1u;
                }
                faces = 1u;
                if (n0 == n1) cancelled = n0 + n1;
                else { keep[idx[p + (n0 > n1 ? 0u : n0)]] = 1; duplicates = n0 + n1 - 1u; }
            }
        }
    }
    const unsigned runs[MEND_RUNS] = {duplicates, cancelled, faces};   // (in the enum's order)
    block_add(runs, head->runs);
}

int mend_device(hipStream_t st, const double *d_soup, const long long *d_cells, long long n_vertices, long long n_tris, DevBuf *out,
                sdf_mend_stats *stats, double kernel_ms[3]) {
    static const char who[] = "sdf_mesh_mend: ";
    if (n_tris < 1 || n_vertices < 1 || 3 * n_tris >= (1ll << 31) || n_vertices >= (1ll << 31))
        return fail(std::string(who) + "the triangle or vertex count is out of range");
    const int vb = bits_for(n_vertices + 1);                           // 0 .. V: V itself marks a collapsed cell
    const int n = (int)n_tris;
    MendHead h_head = {};
    size_t tmp_bytes = 0, need = 0;
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr,
                                                      (unsigned *)nullptr, n, 0, vb + 1, st));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(nullptr, need, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned *)nullptr,
                                                      (unsigned *)nullptr, n, 0, 2 * vb, st));
    tmp_bytes = need > tmp_bytes ? need : tmp_bytes;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n_tris, &tmp_bytes));
    const size_t nt = (size_t)n_tris;
    MendHead *head;
    unsigned long long *hi_soup, *hi_by_lo;                            // hi in soup order (later: in the final order), hi in the order by lo
    unsigned *lo_soup, *lo_sorted, *idx_soup, *idx_by_lo;              // idx_soup: 0 .. T - 1 (later: the final order)
    int *keep, *pos;
    unsigned char *tmp;
    Scratch scratch(st);                                               // (declared after the host copy: it waits for the stream before that goes)
    scratch.part(&head, 1);
    scratch.part(&hi_soup, nt); scratch.part(&hi_by_lo, nt);
    scratch.part(&lo_soup, nt); scratch.part(&lo_sorted, nt);
    scratch.part(&idx_soup, nt); scratch.part(&idx_by_lo, nt);
    scratch.part(&keep, nt); scratch.part(&pos, nt);
    scratch.part(&tmp, tmp_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());

    EventTimer t_keys, t_sorts, t_runs;
    // ---- face and side of every cell ----
    HIPCHK_MSG(who, t_keys.start(st));
    HIPCHK_MSG(who, hipMemsetAsync(head, 0, sizeof(MendHead), st));
    HIPCHK_MSG(who, hipMemsetAsync(keep, 0, nt * 4, st));
    HIPCHK_MSG(who, launch_rows(k_mend_keys, n_tris, st, d_cells, n_tris, n_vertices, vb, hi_soup, lo_soup, idx_soup, head));
    HIPCHK_MSG(who, t_keys.stop(st));
    // ---- by face, then side, then soup order: two stable sorts, the least significant key first ----
    HIPCHK_MSG(who, t_sorts.start(st));
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, lo_soup, lo_sorted, idx_soup, idx_by_lo, n, 0, vb + 1, st));
    HIPCHK_MSG(who, launch_rows(k_mend_gather, n_tris, st, hi_soup, idx_by_lo, n_tris, hi_by_lo));
    unsigned long long *hi_final = hi_soup;                            // (both are free again: the second sort writes into them)
    unsigned *idx_final = idx_soup;
    HIPCHK_MSG(who, hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, hi_by_lo, hi_final, idx_by_lo, idx_final, n, 0, 2 * vb, st));
    HIPCHK_MSG(who, t_sorts.stop(st));
    // ---- one survivor per run with a majority; the survivors ----
    HIPCHK_MSG(who, t_runs.start(st));
    HIPCHK_MSG(who, launch_rows(k_mend_runs, n_tris, st, hi_final, idx_final, lo_soup, n_tris, (unsigned long long)n_vertices << vb, keep, head));
    HIPCHK_MSG(who, hipMemcpyAsync(&h_head, head, sizeof(MendHead), hipMemcpyDeviceToHost, st));       // (lands behind number_flags' wait)
    long long kept = 0;
    if (number_flags(who, "keep flags", st, keep, pos, n_tris, tmp, tmp_bytes, &kept)) return 1;
    if (kept + (long long)(h_head.collapsed + h_head.runs[DUPLICATES] + h_head.runs[CANCELLED]) != n_tris)
        return fail(std::string(who) + "the counts of the runs are inconsistent");
    if (kept > 0) {
        if (out->ensure((size_t)kept * 72)) return 1;
        HIPCHK_MSG(who, select_copy(st, d_soup, keep, pos, n_tris, out->p));
    }
    HIPCHK_MSG(who, t_runs.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, t_keys.ms(&kernel_ms[0]));
    HIPCHK_MSG(who, t_sorts.ms(&kernel_ms[1]));
    HIPCHK_MSG(who, t_runs.ms(&kernel_ms[2]));
    stats->triangles_in = (int64_t)n_tris;
    stats->triangles_out = (int64_t)kept;
    stats->collapsed = (int64_t)h_head.collapsed;
    stats->duplicates = (int64_t)h_head.runs[DUPLICATES];
    stats->cancelled = (int64_t)h_head.runs[CANCELLED];
    stats->faces = (int64_t)h_head.runs[FACES];
    stats->kernel_ms = kernel_ms[0] + kernel_ms[1] + kernel_ms[2];
    return 0;
}

}  // namespace sdfk
