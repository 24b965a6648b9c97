// sdf_components.hip -- the connected shells of a welded mesh (sdf_mesh_components, sdf_mesh_select_shells, ABI 16; DESIGN.md
// section 4h).  tests/components_ref.py is the definition: every cell joins its three welded indices, the label of a vertex is the
// smallest index of its component, shells are numbered by ascending label.  The result is a function of the cells alone.
//
// Labelling.  parent[] holds one 32-bit word per welded vertex; parent[v] <= v always, and a word only ever decreases, through
// integer compare-and-swap or atomicMin.  k_shell_hook gives every cell a lane: it walks to the roots of its three vertices and
// hooks the larger roots under the smallest -- by compare-and-swap ON A ROOT (parent[r] == r expected): a root that another lane
// hooked in the meantime is never overwritten, so no link once made is lost; the compare-and-swap returns the word's true value,
// and the lane goes on from there, strictly downwards.  That is no waiting: no lane ever needs another workgroup to make progress,
// a failed exchange only tells it where the tree has grown.  Plain loads of parent[] may be stale inside a launch (L1 is per CU);
// a stale value is an EARLIER value of the word, which is the vertex itself or one of its true ancestors, so a walk over stale
// words ends at a true ancestor and at worst asks for an exchange that fails.  k_shell_compress then points every vertex at its
// root.  Whether the labelling is complete is decided across a kernel boundary: k_shell_hook counts the cells whose three roots
// were not one (block_count of sdf_block.h), the host reads the counter, and only a full pass that counts none ends the loop.
//
// Numbering: the roots are flagged, a library exclusive scan (hipCUB, like the weld's) numbers them, one lane per vertex and one
// per cell write the shells.  Counts and boxes: integer atomics only, on the ordered keys of sdf_block.h, filter first -- a lane
// accumulates in registers while its run of one shell lasts, a wave whose lanes agree adds up across its lanes, the four waves of a
// workgroup that agree add up in LDS, and one lane issues the atomics; only mixed waves fall back to per-lane atomics.
//
// Selection: a flag per triangle from keep[shell], a library exclusive scan, and a copy with one lane per double of the source soup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>

#include "sdf_block.h"
#include "sdf_components.h"
#include "sdf_prims.h"

namespace sdfk {

constexpr int TALLY_MAX_BLOCKS = 512;                // workgroups that stride over the vertices or the cells (k_shell_tally)

// the apparent root of x: plain loads; where the path is two or more links long the vertex is pointed at its grandparent on the way
// (a true ancestor, by atomicMin: the word only decreases)
__device__ __forceinline__ unsigned shell_root(unsigned *parent, unsigned x) {
    for (;;) {
        const unsigned p = parent[x];
        if (p == x) return x;
        const unsigned g = parent[p];
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

// joins the trees of two apparent roots: the larger is hooked under the smaller if it still is a root; if not, the exchange has
// returned its parent, and the walk goes on from there (max(ra, rb) strictly decreases: the loop ends).  Returns the smaller root.
__device__ __forceinline__ unsigned shell_unite(unsigned *parent, unsigned ra, unsigned rb) {
    while (ra != rb) {
        const unsigned hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const unsigned old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        ra = shell_root(parent, old);
        rb = lo;
    }
    return ra;
}

__global__ __launch_bounds__(256) void k_shell_init(unsigned *__restrict__ parent, long long n) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n) parent[v] = (unsigned)v;
}

// one lane per cell; *n_hooking += the cells whose three apparent roots were not one
__global__ __launch_bounds__(256) void k_shell_hook(const long long *__restrict__ cells, long long n_tris, unsigned *parent, unsigned *n_hooking) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool hooks = false;
    if (i < n_tris) {
        const unsigned ra = shell_root(parent, (unsigned)cells[3 * i]);
        const unsigned rb = shell_root(parent, (unsigned)cells[3 * i + 1]);
        const unsigned rc = shell_root(parent, (unsigned)cells[3 * i + 2]);
        hooks = ra != rb || rb != rc;
        if (hooks) shell_unite(parent, shell_unite(parent, ra, rb), rc);
    }
    const bool is[1] = {hooks};
    block_count(is, n_hooking);
}

// one lane per vertex: to its root (a word another lane has already lowered is a true ancestor too)
__global__ __launch_bounds__(256) void k_shell_compress(unsigned *parent, long long n) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const unsigned p = parent[v];
    unsigned r = p;
    for (;;) {
        const unsigned q = parent[r];
        if (q == r) break;
        r = q;
    }
    if (r < p) atomicMin(parent + v, r);
}

__global__ __launch_bounds__(256) void k_shell_roots(const unsigned *__restrict__ parent, long long n, int *__restrict__ flags) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n) flags[v] = parent[v] == (unsigned)v ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_shell_of_vertex(const unsigned *__restrict__ parent, const int *__restrict__ rank, long long n,
                                                         int *__restrict__ vertex_shell) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < n) vertex_shell[v] = rank[parent[v]];
}

__global__ __launch_bounds__(256) void k_shell_of_cell(const long long *__restrict__ cells, const int *__restrict__ vertex_shell, long long n_tris,
                                                       int *__restrict__ triangle_shell) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_tris) triangle_shell[i] = vertex_shell[cells[3 * i]];
}

// no triangles, no vertices and an empty box per shell: min = the key of +inf, max = the key of -inf
__global__ __launch_bounds__(256) void k_shell_clear(unsigned long long *__restrict__ triangles, unsigned long long *__restrict__ vertices,
                                                     unsigned long long *__restrict__ box, long long n_shells) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_shells) { triangles[i] = 0ull; vertices[i] = 0ull; }
    if (i < 6 * n_shells) {
        box[i] = (i % 6) < 3 ? BOX_EMPTY_LO : BOX_EMPTY_HI;
    }
}

template <bool BOX>
__device__ __forceinline__ void tally_flush(int s, unsigned long long cnt, const unsigned long long *lo, const unsigned long long *hi,
                                            unsigned long long *count, unsigned long long *box) {
    atomicAdd(count + s, cnt);
    if (BOX) {                                                         // (a stale read of the box can only ask for an atomic that was not needed)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            unsigned long long *b = box + 6ll * s;
            if (lo[k] < __atomic_load_n(b + k, __ATOMIC_RELAXED)) atomicMin(b + k, lo[k]);
            if (hi[k] > __atomic_load_n(b + 3 + k, __ATOMIC_RELAXED)) atomicMax(b + 3 + k, hi[k]);
        }
    }
}

// shell[i] of n items (vertices with BOX and their points, or cells): count[shell] += 1, box[shell] takes the point in
template <bool BOX>
__global__ __launch_bounds__(256) void k_shell_tally(const int *__restrict__ shell, long long n, const double *__restrict__ pts,
                                                     unsigned long long *count, unsigned long long *box) {
    int s = -1;
    unsigned long long cnt = 0, lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int k = shell[i];
        if (k != s) {                                                  // the lane's run of one shell has ended
            if (cnt) tally_flush<BOX>(s, cnt, lo, hi, count, box);
            s = k; cnt = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) { lo[c] = ~0ull; hi[c] = 0ull; }
        }
        cnt += 1;
        if (BOX) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned long long key = box_key(pts[3 * i + c]);
                lo[c] = key < lo[c] ? key : lo[c];
                hi[c] = key > hi[c] ? key : hi[c];
            }
        }
    }
    // the wave: do the lanes that hold anything agree with the first of them?
    const unsigned long long have = __ballot(cnt != 0);
    int wave_s = -1;
    if (have != 0ull) {                                                // (uniform)
        const int s0 = __shfl(s, __ffsll((long long)have) - 1);
        if (__ballot(cnt != 0 && s != s0) == 0ull) {
            cnt = wave_sum(cnt);                                       // (a lane that holds nothing holds the identities)
            if (BOX) wave_box_min_max(lo, hi);
            wave_s = s0;
        } else if (cnt) {
            tally_flush<BOX>(s, cnt, lo, hi, count, box);              // a mixed wave: per-lane atomics
        }
    }
    // the four waves meet in LDS; lane 0 adds up the waves that agree and issues the atomics
    __shared__ int w_s[4];
    __shared__ unsigned long long w_v[4][7];
    if ((threadIdx.x & 63u) == 0u) {
        const int w = (int)(threadIdx.x >> 6);
        w_s[w] = wave_s;
        w_v[w][0] = cnt;
#pragma unroll
        for (int c = 0; c < 3; c++) { w_v[w][1 + c] = lo[c]; w_v[w][4 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < 4; w++) {
            if (w_s[w] < 0) continue;
            unsigned long long n_w = w_v[w][0], l[3], h[3];
            for (int c = 0; c < 3; c++) { l[c] = w_v[w][1 + c]; h[c] = w_v[w][4 + c]; }
            for (int x = w + 1; x < 4; x++) {
                if (w_s[x] != w_s[w]) continue;
                n_w += w_v[x][0];
                for (int c = 0; c < 3; c++) {
                    l[c] = w_v[x][1 + c] < l[c] ? w_v[x][1 + c] : l[c];
                    h[c] = w_v[x][4 + c] > h[c] ? w_v[x][4 + c] : h[c];
                }
                w_s[x] = -1;
            }
            tally_flush<BOX>(w_s[w], n_w, l, h, count, box);
        }
    }
}

__global__ __launch_bounds__(256) void k_keep_flags(const int *__restrict__ triangle_shell, const unsigned char *__restrict__ keep, long long n_tris,
                                                    int *__restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_tris) flags[i] = keep[triangle_shell[i]] ? 1 : 0;
}

// one lane per double of the source soup: coalesced reads, a kept triangle's nine doubles go to 9 * pos[triangle]
__global__ __launch_bounds__(256) void k_select_copy(const double *__restrict__ soup, const int *__restrict__ flags, const int *__restrict__ pos,
                                                     long long n_doubles, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_doubles) return;
    const long long t = i / 9;
    if (flags[t]) out[9ll * pos[t] + (i - 9 * t)] = soup[i];
}

hipError_t select_copy(hipStream_t st, const double *d_soup, const int *d_flags, const int *d_pos, long long n_tris, void *d_out) {
    return launch_rows(k_select_copy, 9 * n_tris, st, d_soup, d_flags, d_pos, 9 * n_tris, d_out);
}

size_t shell_block_bytes(long long nv, long long nt, long long k) {
    return align256((size_t)nv * 4) + align256((size_t)nt * 4) + 2 * align256((size_t)k * 8) + align256((size_t)k * 48);
}

ShellParts shell_parts(void *block, long long nv, long long nt, long long k) {
    char *p = static_cast<char *>(block);
    ShellParts s;
    s.vertex_shell = reinterpret_cast<int *>(p); p += align256((size_t)nv * 4);
    s.triangle_shell = reinterpret_cast<int *>(p); p += align256((size_t)nt * 4);
    s.triangles = reinterpret_cast<unsigned long long *>(p); p += align256((size_t)k * 8);
    s.vertices = reinterpret_cast<unsigned long long *>(p); p += align256((size_t)k * 8);
    s.box = reinterpret_cast<unsigned long long *>(p);
    return s;
}

void shell_bounds(const unsigned long long *h_keys, long long n_shells, double *h_bounds) {
    for (long long i = 0; i < 6 * n_shells; i++) h_bounds[i] = box_value(h_keys[i]);
}

int components_label(hipStream_t st, const long long *d_cells, const double *d_points, long long n_tris, long long n_vertices,
                     DevBlock *block, long long *n_shells, int *rounds, double kernel_ms[2]) {
    static const char who[] = "sdf_mesh_components: ";
    block->reset(); *n_shells = 0; *rounds = 0;
    if (n_tris < 1 || n_vertices < 1 || n_tris >= (1ll << 31) || n_vertices >= (1ll << 31))
        return fail(std::string(who) + "the triangle or vertex count is out of range");
    // one merging round and the verifying one are what the scheme needs; the loop allows what root hooking
    // with full compression is bounded by, ceil(log2(max(V, 2))) + 2, and refuses to go on beyond it
    int max_rounds = 2;
    for (long long x = 1; x < n_vertices; x <<= 1) max_rounds += 1;
    if (n_vertices < 2) max_rounds = 3;
    unsigned h_hooking = 0;
    unsigned *parent, *d_hooking;
    int *flags, *rank;
    unsigned char *tmp;
    size_t tmp_bytes = 0;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n_vertices, &tmp_bytes));
    DevBlock kept;                                                     // the block the mesh keeps if all goes well; it goes back on every other path
    Scratch scratch(st);                                               // (declared after the host copies: it waits for the stream before they go)
    scratch.part(&parent, (size_t)n_vertices);
    scratch.part(&flags, (size_t)n_vertices);
    scratch.part(&rank, (size_t)n_vertices);
    scratch.part(&tmp, tmp_bytes);
    scratch.part(&d_hooking, (size_t)max_rounds);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    HIPCHK_MSG(who, hipMemsetAsync(d_hooking, 0, (size_t)max_rounds * 4, st));
    EventTimer t_label, t_number;
    HIPCHK_MSG(who, t_label.start(st));
    HIPCHK_MSG(who, launch_rows(k_shell_init, n_vertices, st, parent, n_vertices));
    int r = 0;
    for (;;) {
        if (r == max_rounds) return fail(std::string(who) + "the labelling did not settle within " + std::to_string(max_rounds) + " rounds");
        HIPCHK_MSG(who, launch_rows(k_shell_hook, n_tris, st, d_cells, n_tris, parent, d_hooking + r));
        HIPCHK_MSG(who, hipMemcpyAsync(&h_hooking, d_hooking + r, 4, hipMemcpyDeviceToHost, st));
        HIPCHK_MSG(who, stream_wait(st));
        r += 1;
        if (h_hooking == 0) break;                                     // a full pass found every cell under one root: parent[] is as the last compression left it
        HIPCHK_MSG(who, launch_rows(k_shell_compress, n_vertices, st, parent, n_vertices));
    }
    HIPCHK_MSG(who, t_label.stop(st));
    HIPCHK_MSG(who, launch_rows(k_shell_roots, n_vertices, st, parent, n_vertices, flags));
    long long k = 0;
    if (number_flags(who, "roots", st, flags, rank, n_vertices, tmp, tmp_bytes, &k)) return 1;
    if (k < 1) return fail(std::string(who) + "the scan of the roots is inconsistent");
    const size_t bytes = shell_block_bytes(n_vertices, n_tris, k);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(bytes) + "): ", kept.alloc(bytes, st));
    const ShellParts sp = shell_parts(kept.as<void>(), n_vertices, n_tris, k);
    HIPCHK_MSG(who, t_number.start(st));
    HIPCHK_MSG(who, launch_rows(k_shell_of_vertex, n_vertices, st, parent, rank, n_vertices, sp.vertex_shell));
    HIPCHK_MSG(who, launch_rows(k_shell_of_cell, n_tris, st, d_cells, sp.vertex_shell, n_tris, sp.triangle_shell));
    HIPCHK_MSG(who, launch_rows(k_shell_clear, 6 * k, st, sp.triangles, sp.vertices, sp.box, k));
    const unsigned v_grid = blocks_of(n_vertices) < TALLY_MAX_BLOCKS ? blocks_of(n_vertices) : TALLY_MAX_BLOCKS;
    const unsigned t_grid = blocks_of(n_tris) < TALLY_MAX_BLOCKS ? blocks_of(n_tris) : TALLY_MAX_BLOCKS;
    HIPCHK_MSG(who, launch_grid(k_shell_tally<true>, v_grid, st, sp.vertex_shell, n_vertices, d_points, sp.vertices, sp.box));
    HIPCHK_MSG(who, launch_grid(k_shell_tally<false>, t_grid, st, sp.triangle_shell, n_tris, nullptr, sp.triangles, nullptr));
    HIPCHK_MSG(who, t_number.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, t_label.ms(&kernel_ms[0]));
    HIPCHK_MSG(who, t_number.ms(&kernel_ms[1]));
    *block = std::move(kept);
    *n_shells = k;
    *rounds = r;
    return 0;
}

int components_select(hipStream_t st, const double *d_soup, long long n_tris, const int *d_triangle_shell, const unsigned char *h_keep,
                      long long n_shells, DevBuf *out, long long *n_kept, double *kernel_ms) {
    static const char who[] = "sdf_mesh_select_shells: ";
    *n_kept = 0;
    if (n_tris < 1 || n_shells < 1 || n_tris >= (1ll << 31)) return fail(std::string(who) + "the triangle or shell count is out of range");
    unsigned char *keep, *tmp;
    int *flags, *pos;
    size_t tmp_bytes = 0;
    HIPCHK_MSG(who, scan_tmp_bytes(st, n_tris, &tmp_bytes));
    Scratch scratch(st);
    scratch.part(&keep, (size_t)n_shells);
    scratch.part(&flags, (size_t)n_tris);
    scratch.part(&pos, (size_t)n_tris);
    scratch.part(&tmp, tmp_bytes);
    HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    HIPCHK_MSG(who, hipMemcpyAsync(keep, h_keep, (size_t)n_shells, hipMemcpyHostToDevice, st));
    EventTimer timer;
    HIPCHK_MSG(who, timer.start(st));
    HIPCHK_MSG(who, launch_rows(k_keep_flags, n_tris, st, d_triangle_shell, keep, n_tris, flags));
    long long kept = 0;
    if (number_flags(who, "flags", st, flags, pos, n_tris, tmp, tmp_bytes, &kept)) return 1;
    if (kept > 0) {
        if (out->ensure((size_t)kept * 72)) return 1;
        HIPCHK_MSG(who, select_copy(st, d_soup, flags, pos, n_tris, out->p));
    }
    HIPCHK_MSG(who, timer.stop(st));
    HIPCHK_MSG(who, stream_wait(st));
    HIPCHK_MSG(who, timer.ms(kernel_ms));
    *n_kept = kept;
    return 0;
}

}  // namespace sdfk
