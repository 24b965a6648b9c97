// sdf_ctx.hip -- the handles of libsdf_hip.so's C ABI that everything else starts from: what the library is (ABI version, build info, the
// devices), a context (its streams, events, call slots, pinned staging, the marching-cubes tables on the device, the tuning switches of
// the environment), a tape (validated, classified -- trigonometric family, interval forms, user closures -- and copied to the device),
// and the marching cubes of a caller-supplied volume, which needs a context and its tables and no tape.
//
// Host code only: the two marching-cubes entry points launch through the launchers of sdf_plain.h, nothing else here launches at all.
// So the unit takes the plain flags, WITHOUT the interpreters' structurizer option (build.units).  -DSDF_BUILD_INFO comes to this unit:
// sdf_build_info() answers with what built the library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "mc_table.h"
#include "sdf_plain.h"
#include "sdf_internal.h"

using namespace sdfk;

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
    if (const char *e = getenv("SDF_MESH_PROF")) { if (atoi(e) && c->prof.ensure(512 + 4096 * 32)) return 1; c->prof_mesh = atoi(e) != 2; }
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

int sdf_tape_set_intervals(sdf_tape *t, int enabled) {
    if (!t) return fail("sdf_tape_set_intervals: tape is NULL");
    t->ia_off = !enabled;
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
