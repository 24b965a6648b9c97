// sdf_comm.hip -- the multi-GPU exchange step inside the library: it drives generate_impl (sdf_generate.hip) and enqueue_skip (sdf_prepass.hip; both
// declared in sdf_internal.h) and k_expand's launcher directly.  No kernels of its own.
//
// One process per GPU.  A rank meshes its contiguous share of the surviving-batch work list into a SLAB (header with
// the counts | per-batch triangle prefix and transform | triangles as 16-byte records in batch-local coordinates, sdf_slab.h
// Tri16: the three along-edge float32 bit for bit + a packed word; the few triangles without that shape as 9 float32 in a raw area), ONE
// ncclAllGather of the equal-sized slabs puts every rank's slab on every rank, and k_expand writes the ordered float64
// soup from them (north_star: "batches shard naturally over the 8 GPUs of one node with an RCCL all-gather of triangle
// buffers over xGMI"; the reference's own parallelism is an ordered thread-pool map over independent batches,
// reference sdf/core.py:131-133).  sdf_amd/dist.py runs the same protocol through torch.distributed (any backend, any
// engine); this is the path for RCCL: the collective is called from here (librccl is dlopen'ed -- a process that never
// creates a communicator never loads it), slabs / gathered slabs / soup live in buffers that persist across steps,
// nothing between "submit" and "wait" goes through the host interpreter, and the host synchronises once per step on
// the gathered headers (every rank reads the same headers, so every rank takes the same decision about a retry).
//
// xGMI on MI355X is point to point (7 links per GPU): an all-gather delivers the 7 remote slabs over 7 links in
// parallel, so the collective's time is one slab over one link; the slabs carry 16 B per triangle (sdf_slab.h; 36 B until r04n)
// instead of the soup's 72 B for that reason.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "sdf_internal.h"

using namespace sdfk;

namespace {

struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

// librccl.so.1 by soname first: a process that already holds one (torch ships its own under the same soname) keeps
// exactly one copy; then the ROCm installation's
static RcclApi *rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {getenv("SDF_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) {
            if (!n || !*n) continue;
            api.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
            api.error = dlerror();
        }
        if (!api.handle) return;
        api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.handle, "ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.handle, "ncclCommInitRank");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.handle, "ncclCommDestroy");
        api.AllGather = (decltype(api.AllGather))dlsym(api.handle, "ncclAllGather");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.handle, "ncclGetErrorString");
        if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather || !api.GetErrorString) {
            api.error = "librccl lacks one of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather / ncclGetErrorString";
            api.handle = nullptr;
        }
    });
    return api.handle ? &api : nullptr;
}

static int rccl_missing() { return fail("RCCL is not available (dlopen of librccl.so.1 failed; SDF_RCCL_LIB names another path)"); }

#define NCCLCHK(x)                                                                                   \
    do {                                                                                             \
        ncclResult_t r_ = (x);                                                                       \
        if (r_ != ncclSuccess) return fail(std::string(#x) + ": " + rccl_api()->GetErrorString(r_)); \
    } while (0)

enum { COMM_MAX_LANES = 2, COMM_MAX_CHUNKS = 8, COMM_MAX_SLABS = 64 };

struct CommLane {
    ncclComm_t comm = nullptr;
    hipStream_t stream = nullptr, cstream = nullptr;      // meshing + expansion / the collectives of a chunked step
    hipEvent_t ev[4] = {};                                // step start, meshing done, gathered, expanded
    hipEvent_t ev_mesh[COMM_MAX_CHUNKS] = {}, ev_gather[COMM_MAX_CHUNKS] = {}, done = nullptr;
    DevBuf mine, gathered, soup, heads, kinds, axes;
    long long *h_heads = nullptr;                         // pinned: COMM_MAX_SLABS x 16 words
    struct sdf_exchange *owner = nullptr;                 // the step in flight on this lane
};

}  // namespace

struct sdf_comm {
    sdf_ctx *ctx = nullptr;
    int device = 0;                                       // (kept apart from ctx: the communicator may outlive a context that is torn down first)
    int rank = 0, world = 1, n_lanes = 1;
    CommLane lanes[COMM_MAX_LANES];
    long long skip_shard_min = 8192;                      // SDF_SKIP_SHARD_MIN: from this many batches on every rank runs the skip test of its share only
                                                          // (k_skip of 8192 batches is ~ 36 us on one GPU; its eighth + an 8 KB all-gather, ~ 20 - 30 us of
                                                          // link latency, is level with that -- below, the whole test on every rank is cheaper; r04: 32768)
    bool skip_shard_forced = false;                       // (the variable is set: a one-rank communicator takes that path too -- tests)
    long long first_cap_tris = 0;                         // SDF_COMM_FIRST_CAP_TRIS: triangle capacity of a job's FIRST step (tests: too small on purpose)
    struct Hint { int64_t cap_items, cap_tris, total; };
    std::map<std::string, Hint> hints;                    // per (tape, grid, chunks): what the last step of the job needed
};

struct sdf_exchange {
    sdf_comm *comm = nullptr;
    int lane = 0;
    sdf_tape *tape = nullptr;
    std::vector<double> axes;
    int nx = 0, ny = 0, nz = 0, bs = 32, sparse = 1, precision = 0, chunks = 1, attempt = 0;
    int64_t cap_items = 0, cap_tris = 0, out_cap = 0;
    size_t slab_bytes = 0;
    std::vector<sdf_mesh *> meshes;
    std::string key;
    bool finished = false;
    sdf_exchange_stats st = {};
};

static void exchange_drop_meshes(sdf_exchange *x) {
    for (sdf_mesh *m : x->meshes) if (m) sdf_mesh_destroy(m);
    x->meshes.clear();
}

// enqueue one attempt of the step on its lane (capacities in x)
static int exchange_submit(sdf_exchange *x) {
    sdf_comm *cm = x->comm;
    sdf_ctx *c = cm->ctx;
    RcclApi *api = rccl_api();
    CommLane &L = cm->lanes[x->lane];
    const int world = cm->world, rank = cm->rank, C = x->chunks, S = world * C;
    const double *X = x->axes.data(), *Y = X + x->nx, *Z = Y + x->ny;
    const int bs = x->bs;
    GridDesc grid;
    const long long nb = grid_desc(x->nx, x->ny, x->nz, bs, grid);
    const size_t sb = SlabLayout(x->cap_items, x->cap_tris).bytes;
    x->slab_bytes = sb;
    if (L.mine.ensure((size_t)C * sb) || L.gathered.ensure((size_t)S * sb) || L.soup.ensure((size_t)std::max<int64_t>(x->out_cap, 1) * 72) ||
        L.heads.ensure((size_t)COMM_MAX_SLABS * 128))
        return 1;
    HIPCHK(hipEventRecord(L.ev[0], L.stream));
    // ---- the skip test: every rank tests its share of the batches, the verdicts are all-gathered (one byte per batch).
    // Only where it pays: on small grids the whole test is cheaper than a collective (512^3, 4096 batches: 19 us). ----
    const unsigned char *d_kinds = nullptr;
    if (x->sparse && (world > 1 || cm->skip_shard_forced) && nb >= cm->skip_shard_min && nb > 0) {
        const long long piece = ((nb + world - 1) / world + 255) & ~255ll;     // (whole 256-byte pieces: every rank's part of the in-place gather starts aligned)
        if (L.kinds.ensure((size_t)piece * world) || L.axes.ensure((size_t)(x->nx + x->ny + x->nz) * 8)) return 1;
        HIPCHK(hipMemcpyAsync(L.axes.p, X, (size_t)(x->nx + x->ny + x->nz) * 8, hipMemcpyHostToDevice, L.stream));
        const long long b0 = std::min<long long>(nb, piece * rank), b1 = std::min<long long>(nb, piece * (rank + 1));
        if (enqueue_skip(x->tape, (const double *)L.axes.p, x->nx, x->ny, x->nz, bs, (int)b0, (int)b1, x->precision, (unsigned char *)L.kinds.p, L.stream))
            return 1;
        NCCLCHK(api->AllGather((const unsigned char *)L.kinds.p + (size_t)piece * rank, L.kinds.p, (size_t)piece, ncclUint8, L.comm, L.stream));   // in place
        d_kinds = (const unsigned char *)L.kinds.p;
    }
    // ---- mesh the rank's shard(s) into slabs, gather them ----
    x->meshes.assign((size_t)C, nullptr);
    for (int j = 0; j < C; j++) {
        sdf_mesh *m = new sdf_mesh();
        m->ctx = c;
        x->meshes[(size_t)j] = m;
        unsigned char *mine = (unsigned char *)L.mine.p + (size_t)j * sb;
        GenCall call = gen_call(x->tape, X, x->nx, Y, x->ny, Z, x->nz, bs, x->sparse, (int64_t)rank * C + j, (int64_t)S, x->precision);
        call.dest = GenCall::SLAB; call.d_out = mine; call.cap_items = x->cap_items; call.cap_tris = x->cap_tris;
        call.collected = true; call.lane = L.stream; call.d_kinds = d_kinds;
        if (generate_impl(m, call)) return 1;
        unsigned char *g = (unsigned char *)L.gathered.p + (size_t)j * world * sb;
        if (C == 1) {
            HIPCHK(hipEventRecord(L.ev[1], L.stream));
            NCCLCHK(api->AllGather(mine, g, sb, ncclUint8, L.comm, L.stream));
        } else {   // the gather of shard j runs on the lane's second stream, under the meshing of shard j + 1
            HIPCHK(hipEventRecord(L.ev_mesh[j], L.stream));
            if (j == C - 1) HIPCHK(hipEventRecord(L.ev[1], L.stream));
            HIPCHK(hipStreamWaitEvent(L.cstream, L.ev_mesh[j], 0));
            NCCLCHK(api->AllGather(mine, g, sb, ncclUint8, L.comm, L.cstream));
            HIPCHK(hipEventRecord(L.ev_gather[j], L.cstream));
        }
    }
    if (C > 1) for (int j = 0; j < C; j++) HIPCHK(hipStreamWaitEvent(L.stream, L.ev_gather[j], 0));
    HIPCHK(hipEventRecord(L.ev[2], L.stream));
    // ---- gathered slabs -> the ordered float64 soup; slab (rank r, shard j) is piece r * C + j of the work list ----
    SlabPtrs ptrs = {};
    for (int r = 0; r < world; r++)
        for (int j = 0; j < C; j++) ptrs.p[r * C + j] = (const unsigned char *)L.gathered.p + ((size_t)j * world + r) * sb;
    if (x->cap_items > 0 && x->out_cap > 0) {
        const unsigned long long blocks = ((unsigned long long)x->out_cap + 255ull) / 256ull;
        if (blocks > 0x7fffffffull) return fail("sdf_generate_sharded_async: soup capacity too large for one expansion launch");
        HIPCHK((hipError_t)sdf_launch_expand(L.stream, ptrs, S, (long long)x->cap_items, (long long)x->cap_tris, (double *)L.soup.p, (unsigned long long)x->out_cap));
    }
    HIPCHK(hipEventRecord(L.ev[3], L.stream));
    HIPCHK((hipError_t)sdf_launch_collect_headers(L.stream, ptrs, S, (long long *)L.heads.p));
    HIPCHK(hipMemcpyAsync(L.h_heads, L.heads.p, (size_t)S * 128, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(hipEventRecord(L.done, L.stream));
    L.owner = x;
    return 0;
}

// first-call capacities: a shard is a contiguous piece of the work list, at most 1 / (world * chunks) of ALL batches;
// triangles: a guess (4096 per batch of the shard) within 8 GB for the gathered slabs + the soup (72 B) together (a triangle of a slab is a 16-byte record plus 1/128 of a 36-byte raw entry: 89 B with the soup's 72) -- a
// slab that is too small is flagged in its header, the headers carry the exact need, and the step is repeated once with
// that.  The capacities decide the SIZE of the collective, so they must come out the same on every rank: nothing
// rank-local (free memory, say) may enter the formula.
static void exchange_first_caps(sdf_exchange *x, long long nb) {
    const long long S = (long long)x->comm->world * x->chunks;
    x->cap_items = (nb + S - 1) / S + 1;
    const unsigned long long budget = 8ull << 30;
    x->cap_tris = (int64_t)std::max<unsigned long long>(std::min<unsigned long long>(4096ull * (unsigned long long)x->cap_items, budget / (89ull * (unsigned long long)S)), 1ull << 16);
    if (x->comm->first_cap_tris > 0) x->cap_tris = x->comm->first_cap_tris;
    x->out_cap = (int64_t)S * x->cap_tris;
}

extern "C" {

int sdf_comm_available(void) {
    if (rccl_api()) return 1;
    rccl_missing();
    return 0;
}

int sdf_comm_unique_id(void *out_id) {
    if (!out_id) return fail("sdf_comm_unique_id: NULL argument");
    RcclApi *api = rccl_api();
    if (!api) return rccl_missing();
    static_assert(sizeof(ncclUniqueId) == SDF_COMM_ID_BYTES, "ncclUniqueId");
    ncclUniqueId id;
    NCCLCHK(api->GetUniqueId(&id));
    memcpy(out_id, &id, sizeof(id));
    return 0;
}

int sdf_comm_destroy(sdf_comm *cm) {
    if (!cm) return 0;
    (void)hipSetDevice(cm->device);
    RcclApi *api = rccl_api();
    for (int l = 0; l < COMM_MAX_LANES; l++) {
        CommLane &L = cm->lanes[l];
        if (L.stream) (void)stream_wait(L.stream);
        if (L.cstream) (void)stream_wait(L.cstream);
        if (L.comm && api) (void)api->CommDestroy(L.comm);
        for (DevBuf *b : {&L.mine, &L.gathered, &L.soup, &L.heads, &L.kinds, &L.axes}) b->release();
        for (hipEvent_t e : L.ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : L.ev_mesh) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : L.ev_gather) if (e) (void)hipEventDestroy(e);
        if (L.done) (void)hipEventDestroy(L.done);
        if (L.h_heads) (void)hipHostFree(L.h_heads);
        if (L.stream) (void)hipStreamDestroy(L.stream);
        if (L.cstream) (void)hipStreamDestroy(L.cstream);
    }
    delete cm;
    return 0;
}

static int comm_init(sdf_comm *cm, const void *ids, int n_lanes) {
    RcclApi *api = rccl_api();
    for (int l = 0; l < n_lanes; l++) {
        CommLane &L = cm->lanes[l];
        HIPCHK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&L.cstream, hipStreamNonBlocking));
        for (auto &e : L.ev) HIPCHK(hipEventCreate(&e));
        for (auto &e : L.ev_mesh) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : L.ev_gather) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        HIPCHK(host_malloc((void **)&L.h_heads, (size_t)COMM_MAX_SLABS * 128));
        ncclUniqueId id;
        memcpy(&id, (const char *)ids + (size_t)l * SDF_COMM_ID_BYTES, sizeof(id));
        NCCLCHK(api->CommInitRank(&L.comm, cm->world, id, cm->rank));
    }
    return 0;
}

int sdf_comm_create(sdf_ctx *c, const void *ids, int n_lanes, int rank, int world, sdf_comm **out) {
    if (!c || !ids || !out) return fail("sdf_comm_create: NULL argument");
    *out = nullptr;
    if (n_lanes < 1 || n_lanes > COMM_MAX_LANES) return fail("sdf_comm_create: 1 or 2 lanes");
    if (world < 1 || rank < 0 || rank >= world) return fail("sdf_comm_create: bad rank / world size");
    if (world > COMM_MAX_SLABS) return fail("sdf_comm_create: at most 64 ranks (one slab per rank and shard, 64 slabs per expansion)");
    if (!rccl_api()) return rccl_missing();
    HIPCHK(set_device(c->device));
    sdf_comm *cm = new sdf_comm();
    cm->ctx = c; cm->device = c->device; cm->rank = rank; cm->world = world; cm->n_lanes = n_lanes;
    if (const char *e = getenv("SDF_SKIP_SHARD_MIN")) { cm->skip_shard_min = atoll(e); cm->skip_shard_forced = true; }
    if (const char *e = getenv("SDF_COMM_FIRST_CAP_TRIS")) cm->first_cap_tris = atoll(e);
    if (comm_init(cm, ids, n_lanes)) {
        const std::string keep = g_err;
        sdf_comm_destroy(cm);
        g_err = keep;
        return 1;
    }
    *out = cm;
    return 0;
}

int sdf_exchange_destroy(sdf_exchange *x) {
    if (!x) return 0;
    CommLane &L = x->comm->lanes[x->lane];
    (void)hipSetDevice(x->comm->device);   // (not ctx->device: the communicator may outlive its context)
    if (L.owner == x) { (void)stream_wait(L.stream); (void)stream_wait(L.cstream); L.owner = nullptr; }
    exchange_drop_meshes(x);
    delete x;
    return 0;
}

int sdf_generate_sharded_async(sdf_comm *cm, sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz,
                               int bs, int sparse, int precision, int chunks, int lane, sdf_exchange **out) {
    if (!cm || !t || !X || !Y || !Z || !out) return fail("sdf_generate_sharded_async: NULL argument");
    *out = nullptr;
    if (t->ctx != cm->ctx) return fail("sdf_generate_sharded_async: tape and communicator belong to different contexts");
    if (t->n_extern) return fail("sdf_generate_sharded_async: the tape reads user closures (L_EXTERN): shard it through sdf_generate_field + the host protocol (sdf_amd/dist.py)");
    if (bs < 1 || bs > 32) return fail("sdf_generate_sharded_async: batch_size must be in 1..32");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_generate_sharded_async: bad precision");
    if (nx < 0 || ny < 0 || nz < 0) return fail("sdf_generate_sharded_async: negative axis length");
    if (lane < 0 || lane >= cm->n_lanes) return fail("sdf_generate_sharded_async: no such lane");
    if (cm->lanes[lane].owner) return fail("sdf_generate_sharded_async: the lane still holds a step (sdf_exchange_wait / sdf_exchange_destroy it first)");
    if ((size_t)(nx + ny + nz) * 8 > SDF_STAGE_BYTES - 256) return fail("sdf_generate_sharded_async: axes too long for the staging slot");
    HIPCHK(set_device(cm->device));
    sdf_exchange *x = new sdf_exchange();
    x->comm = cm; x->lane = lane; x->tape = t;
    x->axes.assign(X, X + nx); x->axes.insert(x->axes.end(), Y, Y + ny); x->axes.insert(x->axes.end(), Z, Z + nz);
    x->nx = nx; x->ny = ny; x->nz = nz; x->bs = bs; x->sparse = sparse ? 1 : 0; x->precision = precision;
    x->chunks = std::max(1, std::min(std::min(chunks, (int)COMM_MAX_CHUNKS), COMM_MAX_SLABS / cm->world));
    char key[160];
    // (keyed by the tape's CONTENT, not its address: a freed tape's address is recycled by the allocator, differently on every
    // rank, and a capacity inherited on one rank only would give the ranks slabs of different sizes in one all-gather)
    snprintf(key, sizeof key, "%016llx:%u:%d:%d:%d:%d:%d:%d:%d", t->content_hash, t->n_words, nx, ny, nz, bs, x->sparse, precision, x->chunks);
    x->key = key;
    GridDesc grid;
    const long long nb = grid_desc(nx, ny, nz, bs, grid);
    auto it = cm->hints.find(x->key);
    if (it != cm->hints.end()) {
        x->cap_items = it->second.cap_items; x->cap_tris = it->second.cap_tris;
        x->out_cap = it->second.total + it->second.total / 8 + 4096;
    } else {
        exchange_first_caps(x, nb);
    }
    if (exchange_submit(x)) {
        const std::string keep = g_err;
        sdf_exchange_destroy(x);
        g_err = keep;
        return 1;
    }
    *out = x;
    return 0;
}

int sdf_exchange_wait(sdf_exchange *x, void **d_soup, int64_t *n_tris) {
    if (!x) return fail("sdf_exchange_wait: NULL argument");
    sdf_comm *cm = x->comm;
    CommLane &L = cm->lanes[x->lane];
    HIPCHK(set_device(cm->device));
    while (!x->finished) {
        if (L.owner != x) return fail("sdf_exchange_wait: the step is not in flight");
        HIPCHK(event_wait(L.done));
        const int world = cm->world, C = x->chunks, S = world * C;
        std::vector<long long> heads(L.h_heads, L.h_heads + (size_t)S * 16);
        float ms_mesh = 0, ms_x = 0, ms_e = 0, ms_t = 0;
        HIPCHK(hipEventElapsedTime(&ms_mesh, L.ev[0], L.ev[1]));
        HIPCHK(hipEventElapsedTime(&ms_x, L.ev[1], L.ev[2]));
        HIPCHK(hipEventElapsedTime(&ms_e, L.ev[2], L.ev[3]));
        HIPCHK(hipEventElapsedTime(&ms_t, L.ev[0], L.ev[3]));
        // the meshes' own counters are in the headers; the handles only kept the calls' device buffers alive
        for (sdf_mesh *m : x->meshes) if (m && sdf_mesh_wait(m, nullptr)) return 1;
        exchange_drop_meshes(x);
        L.owner = nullptr;
        int64_t total = 0, need_items = 0, need_tris = 0, flags = 0;
        for (int s = 0; s < S; s++) {
            const long long *h = &heads[(size_t)s * 16];
            total += h[0]; need_tris = std::max<int64_t>(need_tris, std::max(h[0], h[11])); need_items = std::max<int64_t>(need_items, h[1]); flags |= h[2];   // (h[11]: capacity a too-small raw area asks for)
        }
        if (flags & 2) return fail("sdf_exchange_wait: a rank reported a look-back timeout");
        const bool ok = !flags && need_items <= x->cap_items && need_tris <= x->cap_tris && total <= x->out_cap;
        if (!ok) {
            if (x->attempt >= 5) return fail("sdf_exchange_wait: slab capacities did not converge");
            x->attempt++;
            x->cap_items = std::max<int64_t>(x->cap_items, need_items + need_items / 8 + 16);
            x->cap_tris = std::max<int64_t>(x->cap_tris, need_tris + need_tris / 64 + 1024);
            x->out_cap = total + total / 8 + 4096;
            if (exchange_submit(x)) return 1;
            continue;
        }
        // (the same job -- the key holds the tape's content and the grid -- needs the same capacities again: the slack only
        // rounds up; a slab that is too small after all is flagged and the step repeated)
        cm->hints[x->key] = sdf_comm::Hint{need_items + need_items / 8 + 16, need_tris + need_tris / 64 + 1024, total};
        sdf_exchange_stats &st = x->st;
        st = sdf_exchange_stats{};
        GridDesc grid;
        st.n_batches = (int64_t)grid_desc(x->nx, x->ny, x->nz, x->bs, grid);
        st.n_skipped = st.n_batches - heads[9];
        st.n_grid_voxels = (int64_t)x->nx * x->ny * x->nz;
        st.n_triangles = total; st.n_retries = x->attempt; st.chunks = C; st.world = world; st.slab_bytes = (int64_t)x->slab_bytes;
        for (int s = 0; s < S; s++) {
            const long long *h = &heads[(size_t)s * 16];
            st.n_empty += h[3]; st.n_nonempty += h[4]; st.n_eval_voxels += h[5]; st.n_ambiguous_cells += h[6];
            st.n_sampled_voxels += h[7]; st.n_pruned_instrs += h[8];
            st.per_rank_triangles[s / C] += h[0];
        }
        st.ms_mesh = ms_mesh; st.ms_exchange = ms_x; st.ms_expand = ms_e; st.ms_total = ms_t;
        x->finished = true;
    }
    if (d_soup) *d_soup = L.soup.p;
    if (n_tris) *n_tris = x->st.n_triangles;
    return 0;
}

int sdf_exchange_stats_get(sdf_exchange *x, sdf_exchange_stats *out) {
    if (!x || !out) return fail("sdf_exchange_stats_get: NULL argument");
    if (!x->finished && sdf_exchange_wait(x, nullptr, nullptr)) return 1;
    *out = x->st;
    return 0;
}

int sdf_skip_kinds(sdf_tape *t, const double *X, int nx, const double *Y, int ny, const double *Z, int nz, int bs, int64_t b_begin,
                   int64_t b_end, int precision, void *d_kinds) {
    if (!t || !X || !Y || !Z || !d_kinds) return fail("sdf_skip_kinds: NULL argument");
    if (t->n_extern) return fail("sdf_skip_kinds: the tape reads user closures (L_EXTERN)");
    if (bs < 1 || bs > 32) return fail("sdf_skip_kinds: batch_size must be in 1..32");
    if (precision != SDF_PRECISION_F64 && precision != SDF_PRECISION_F32) return fail("sdf_skip_kinds: bad precision");
    if (nx < 0 || ny < 0 || nz < 0) return fail("sdf_skip_kinds: negative axis length");
    GridDesc grid;
    int nb = 0;
    if (grid_batches(nx, ny, nz, bs, "sdf_skip_kinds", grid, nb)) return 1;
    if (b_begin < 0 || b_end < b_begin || b_end > nb) return fail("sdf_skip_kinds: batch range outside the grid");
    if (b_begin == b_end) return 0;
    sdf_ctx *c = t->ctx;
    HIPCHK(set_device(c->device));
    if (c->scratch_in.ensure((size_t)(nx + ny + nz) * 8)) return 1;
    double *dX = (double *)c->scratch_in.p;
    HIPCHK(hipMemcpyAsync(dX, X, (size_t)nx * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dX + nx, Y, (size_t)ny * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dX + nx + ny, Z, (size_t)nz * 8, hipMemcpyHostToDevice, c->stream));
    if (enqueue_skip(t, dX, nx, ny, nz, bs, (int)b_begin, (int)b_end, precision, (unsigned char *)d_kinds, c->stream)) return 1;
    HIPCHK(stream_wait(c->stream));     // (the axes' staging buffer belongs to the context)
    return 0;
}

int sdf_memcpy_to_host(sdf_ctx *c, void *h_dst, const void *d_src, size_t bytes) {
    if (!c || (bytes && (!h_dst || !d_src))) return fail("sdf_memcpy_to_host: NULL argument");
    if (!bytes) return 0;
    HIPCHK(set_device(c->device));
    return copy_to_host(c, h_dst, d_src, bytes);
}

}  // extern "C"
