// sdf_probe_out.hip -- the host entries of the field probes: what takes a tape to a finished mesh or to an image --
// field normals, the wall thickness and the curvature at the welded vertices, the deviation of the triangles from the field and the
// vertices snapped onto it, the support rays, the sphere-traced image.  Host code only: it launches through the launchers of sdf_normals.h,
// sdf_thickness.h, sdf_curvature.h, sdf_deviation.h, sdf_supports.h, sdf_render.h and sdf_plain.h, built WITHOUT the interpreters' structurizer option
// (build.units).  Every entry returns 0: done, 1: HIP error, 2: refused (nothing allocated, nothing launched); sdf_last_error says why.
// What the entries share stands in front of them, and an entry uses it where its own lines stood.
#include <cmath>
#include <cstring>

#include "sdf_internal.h"
#include "sdf_curvature.h"
#include "sdf_deviation.h"
#include "sdf_normals.h"
#include "sdf_plain.h"
#include "sdf_render.h"
#include "sdf_supports.h"
#include "sdf_thickness.h"

using namespace sdfk;

static int refuse(const char *who, const std::string &why) { fail(std::string(who) + ": " + why); return 2; }
#define REFUSE(why) return refuse(__func__, why)

// The events around a launch and, behind the entry's copies, the wait and the kernel's time; `timer` is the entry's EventTimer.
// Macros, so that HIPCHK_FN still names the entry and quotes the call that failed.
#define TIMED_LAUNCH(st, launch) do { HIPCHK_FN(timer.start(st)); launch; HIPCHK_FN(timer.stop(st)); } while (0)
#define TIMED_RESULTS(st, to) do { HIPCHK_FN(stream_wait(st)); HIPCHK_FN(timer.ms(to)); } while (0)

// the mesh and the tape of a call, both not NULL; extern_why: why this entry cannot serve a tape with user closures.  0 or 2
static int probe_refused(const char *who, const sdf_mesh *m, const sdf_tape *t, bool need_weld, const char *extern_why) {
    if (need_weld && m->weld_n < 0) return refuse(who, "call sdf_mesh_weld first");
    if (t->ctx != m->ctx) return refuse(who, "the tape and the mesh belong to different contexts");
    if (t->n_extern) return refuse(who, std::string("the tape reads user closures (L_EXTERN): ") + extern_why);
    return 0;
}

// the parameters of a ray march (thickness; supports, whose rays end at the bed: t_far = +inf); 0 when they are in order
static int march_refused(const char *who, double start, double min_step, double step_scale, double t_far, int max_steps, int refine) {
    if (!(start > 0.0)) return refuse(who, "start must be positive");
    if (!(min_step > 0.0)) return refuse(who, "min_step must be positive");
    if (!(step_scale > 0.0 && step_scale <= 1.0)) return refuse(who, "step_scale must lie in (0, 1]");
    if (t_far < start) return refuse(who, "t_far lies before start");
    if (max_steps < 1) return refuse(who, "max_steps must be at least 1");
    if (refine < 0) return refuse(who, "refine must not be negative");
    return 0;
}

// what sdf_mesh_support_rays leaves behind: one device block per direction that has rays
struct sdf_support_rays {
    sdf_ctx *ctx = nullptr;
    std::vector<SupportRaysDir> dirs;
};

extern "C" {

// ---- the indexed export: field normals at the welded vertices ----
static thread_local double g_normals_kernel_ms = 0.0;

int sdf_mesh_vertex_normals(sdf_mesh *m, sdf_tape *t, double eps, double *h_normals, int64_t *n_flat) {
    if (!m || !t || !n_flat) REFUSE("NULL argument");
    if (!(std::isfinite(eps) && eps > 0.0)) REFUSE("eps must be finite and positive");
    // (this entry alone asks about closures BEFORE the weld, so it spells its three refusals out)
    if (t->n_extern) REFUSE("the tape reads user closures (L_EXTERN): take the normals over sdf_eval_points_extern_host");
    if (m->weld_n < 0) REFUSE("call sdf_mesh_weld first");
    if (t->ctx != m->ctx) REFUSE("the tape and the mesh belong to different contexts");
    sdf_ctx *c = m->ctx;
    const long long nu = m->weld_n;
    *n_flat = 0;
    if (nu == 0) { m->nrm_valid = true; m->nrm_model = t->content_hash; m->nrm_eps = eps; m->nrm_flat = 0; return 0; }
    HIPCHK(set_device(c->device));
    if (!(m->nrm_valid && m->nrm_model == t->content_hash && m->nrm_eps == eps)) {
        m->nrm_valid = false;
        static const char who[] = "sdf_mesh_vertex_normals: ";
        if (!m->nrm) HIPCHK_MSG(std::string(who) + "hipMalloc(" + std::to_string((size_t)nu * 24 + 8) + "): ", m->nrm.alloc((size_t)nu * 24 + 8, c->stream));
        double *nrm = m->nrm.as<double>();
        unsigned long long *d_flat = reinterpret_cast<unsigned long long *>(nrm + 3 * nu);
        EventTimer timer;
        HIPCHK_MSG(who, hipMemsetAsync(d_flat, 0, 8, c->stream));
        HIPCHK_MSG(who, timer.start(c->stream));
        HIPCHK_MSG(who, (hipError_t)launch_vertex_normals(c->stream, t->d_code, t->d_c64, t->full, m->weld_pts.as<double>(), nu, eps, nrm, d_flat));
        HIPCHK_MSG(who, timer.stop(c->stream));
        // (the count lands in the mesh, not on this stack: a call that fails on the way out leaves no copy in flight to a dead frame)
        HIPCHK_MSG(who, hipMemcpyAsync(&m->nrm_flat, d_flat, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK_MSG(who, stream_wait(c->stream));
        HIPCHK_MSG(who, timer.ms(&g_normals_kernel_ms));
        m->nrm_valid = true; m->nrm_model = t->content_hash; m->nrm_eps = eps;
    }
    *n_flat = (int64_t)m->nrm_flat;
    if (h_normals) return copy_to_host(c, h_normals, m->nrm.as<double>(), (size_t)nu * 24);
    return 0;
}

double sdf_mesh_normals_last_kernel_ms(void) { return g_normals_kernel_ms; }

// ---- the wall thickness at the welded vertices: inward rays through the solid ----
static thread_local double g_thickness_kernel_ms = 0.0;

int sdf_mesh_vertex_thickness(sdf_mesh *m, sdf_tape *t, const double *params6, int max_steps, int refine, double *h_thickness,
                              uint8_t *h_status, int32_t *h_steps) {
    if (!m || !t || !params6 || !h_thickness || !h_status || !h_steps) REFUSE("NULL argument");
    if (probe_refused(__func__, m, t, true, "every step of every ray would need a host round trip")) return 2;
    for (int i = 0; i < 6; i++) if (!std::isfinite(params6[i])) REFUSE("the parameters are not finite");
    ThicknessArgs a;
    a.normal_eps = params6[0]; a.start = params6[1]; a.min_step = params6[2]; a.t_far = params6[3]; a.step_scale = params6[4];
    a.max_steps = max_steps; a.refine = refine;
    if (!(a.normal_eps > 0.0)) REFUSE("normal_eps must be positive");
    if (march_refused(__func__, a.start, a.min_step, a.step_scale, a.t_far, max_steps, refine)) return 2;
    const long long nu = m->weld_n;
    if (nu == 0) return 0;
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    hipStream_t st = c->stream;
    double *thick;
    int32_t *steps;
    uint8_t *status;
    Scratch scratch(st);
    scratch.part(&thick, (size_t)nu); scratch.part(&steps, (size_t)nu); scratch.part(&status, (size_t)nu);
    EventTimer timer;
    HIPCHK_MSG("sdf_mesh_vertex_thickness: hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    TIMED_LAUNCH(st, HIPCHK_FN((hipError_t)launch_vertex_thickness(st, t->d_code, t->d_c64, t->full, m->weld_pts.as<double>(), nu, a, thick, status, steps)));
    HIPCHK_FN(hipMemcpyAsync(h_thickness, thick, (size_t)nu * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_status, status, (size_t)nu, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_steps, steps, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    TIMED_RESULTS(st, &g_thickness_kernel_ms);
    return 0;
}

double sdf_mesh_thickness_last_kernel_ms(void) { return g_thickness_kernel_ms; }

// ---- the curvature of the field's level set at the welded vertices: mean, Gaussian, principal ----
static thread_local double g_curvature_kernel_ms = 0.0;

int sdf_mesh_vertex_curvature(sdf_mesh *m, sdf_tape *t, double eps, double *h_curv4, uint8_t *h_status, int64_t *h_counts3) {
    if (!m || !t || !h_curv4 || !h_status || !h_counts3) REFUSE("NULL argument");
    if (probe_refused(__func__, m, t, true, "take the curvature over sdf_eval_points_extern_host")) return 2;
    if (!(std::isfinite(eps) && eps > 0.0)) REFUSE("eps must be finite and positive");
    const long long nu = m->weld_n;
    for (int k = 0; k < 3; k++) h_counts3[k] = 0;
    if (nu == 0) return 0;
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    hipStream_t st = c->stream;
    double *curv;
    unsigned long long *counts;
    uint8_t *status;
    Scratch scratch(st);
    scratch.part(&curv, (size_t)nu * 4); scratch.part(&counts, (size_t)3); scratch.part(&status, (size_t)nu);
    EventTimer timer;
    HIPCHK_MSG("sdf_mesh_vertex_curvature: hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    HIPCHK_FN(hipMemsetAsync(counts, 0, 24, st));
    TIMED_LAUNCH(st, HIPCHK_FN((hipError_t)launch_vertex_curvature(st, t->d_code, t->d_c64, t->full, m->weld_pts.as<double>(), nu, eps, curv, status, counts)));
    HIPCHK_FN(hipMemcpyAsync(h_curv4, curv, (size_t)nu * 32, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_status, status, (size_t)nu, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_counts3, counts, 24, hipMemcpyDeviceToHost, st));
    TIMED_RESULTS(st, &g_curvature_kernel_ms);
    return 0;
}

double sdf_mesh_curvature_last_kernel_ms(void) { return g_curvature_kernel_ms; }

// ---- a mesh held to the field: the deviation of every triangle, the welded vertices snapped onto the zero set ----
static thread_local double g_deviation_kernel_ms = 0.0;

int sdf_mesh_triangle_deviation(sdf_mesh *m, sdf_tape *t, int order, double *h_dev, int32_t *h_at, double *h_sumsq) {
    if (!m || !t || !h_dev || !h_at || !h_sumsq) REFUSE("NULL argument");
    if (probe_refused(__func__, m, t, false, "take the deviation over sdf_eval_points_extern_host")) return 2;
    if (order < 1 || order > 8) REFUSE("order must lie in 1 .. 8");
    MESH_READY(m);
    const long long nt = (long long)m->st.n_triangles;
    if (nt >= (1ll << 31)) REFUSE("2^31 or more triangles");
    if (nt == 0) return 0;
    MESH_SOUP_READY(m);
    sdf_ctx *c = m->ctx;
    HIPCHK(set_device(c->device));
    hipStream_t st = c->stream;
    double *dev, *sumsq;
    int32_t *at;
    Scratch scratch(st);
    scratch.part(&dev, (size_t)nt); scratch.part(&sumsq, (size_t)nt); scratch.part(&at, (size_t)nt);
    EventTimer timer;
    HIPCHK_MSG("sdf_mesh_triangle_deviation: hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
    TIMED_LAUNCH(st, HIPCHK_FN((hipError_t)launch_triangle_deviation(st, t->d_code, t->d_c64, t->full, (const double *)mesh_soup(m), nt, order, dev, at, sumsq)));
    HIPCHK_FN(hipMemcpyAsync(h_dev, dev, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_at, at, (size_t)nt * 4, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_sumsq, sumsq, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
    TIMED_RESULTS(st, &g_deviation_kernel_ms);
    return 0;
}

double sdf_mesh_deviation_last_kernel_ms(void) { return g_deviation_kernel_ms; }

int sdf_mesh_snap(sdf_mesh *m, sdf_tape *t, const double *params4, int iters, sdf_mesh **out, double *h_points, uint8_t *h_status,
                  double *h_residual, int32_t *h_evals, sdf_snap_stats *stats) {
    if (!m || !t || !params4 || !out || !stats) REFUSE("NULL argument");
    if (probe_refused(__func__, m, t, true, "every pass would need a host round trip")) return 2;
    for (int i = 0; i < 4; i++) if (!std::isfinite(params4[i])) REFUSE("the parameters are not finite");
    SnapArgs a;
    a.eps = params4[0]; a.two_eps = 2.0 * params4[0]; a.tol = params4[1]; a.max_move = params4[2]; a.iters = iters;
    if (!(a.eps > 0.0)) REFUSE("eps must be positive");
    if (!(a.tol >= 0.0)) REFUSE("tol must not be negative");
    if (!(a.max_move >= 0.0)) REFUSE("max_move must not be negative");
    if (iters < 1) REFUSE("iters must be at least 1");
    const long long nu = m->weld_n, nt = (long long)m->st.n_triangles;
    sdf_snap_stats got = sdf_snap_stats();
    got.vertices = (int64_t)nu;
    DevBuf soup;                                                       // the moved vertices' own soup: the new mesh's `out`
    if (nu > 0 && nt > 0) {                                            // (nothing to move: a mesh of 0 triangles, no launch)
        sdf_ctx *c = m->ctx;
        HIPCHK(set_device(c->device));
        hipStream_t st = c->stream;
        double *q, *residual;
        int32_t *evals;
        uint8_t *status;
        Scratch scratch(st);
        scratch.part(&q, (size_t)nu * 3); scratch.part(&residual, (size_t)nu); scratch.part(&evals, (size_t)nu); scratch.part(&status, (size_t)nu);
        std::vector<uint8_t> codes((size_t)nu);
        EventTimer timer;
        HIPCHK_MSG("sdf_mesh_snap: hipMalloc(" + std::to_string(scratch.bytes) + "): ", scratch.alloc());
        if (soup.ensure((size_t)nt * 72)) return 1;
        // (from here on a failure hands the soup back: the scratch block drains the stream before it goes)
        static const char who[] = "sdf_mesh_snap: ";
        auto run = [&]() -> int {
            HIPCHK_MSG(who, timer.start(st));
            HIPCHK_MSG(who, (hipError_t)launch_vertex_snap(st, t->d_code, t->d_c64, t->full, m->weld_pts.as<double>(), nu, a, q, status, residual, evals));
            HIPCHK_MSG(who, timer.stop(st));
            launch_k_gather_soup(dim3(blocks_of(9 * nt)), dim3(256), st, q, m->weld_inv.as<long long>(), 9 * nt, (double *)soup.p);
            HIPCHK_MSG(who, hipGetLastError());
            HIPCHK_MSG(who, hipMemcpyAsync(codes.data(), status, (size_t)nu, hipMemcpyDeviceToHost, st));
            if (h_points) HIPCHK_MSG(who, hipMemcpyAsync(h_points, q, (size_t)nu * 24, hipMemcpyDeviceToHost, st));
            if (h_residual) HIPCHK_MSG(who, hipMemcpyAsync(h_residual, residual, (size_t)nu * 8, hipMemcpyDeviceToHost, st));
            if (h_evals) HIPCHK_MSG(who, hipMemcpyAsync(h_evals, evals, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
            return 0;
        };
        const int rc = run();
        const hipError_t e = stream_wait(st);                          // (before `codes` goes, whatever the copies said)
        if (rc || e != hipSuccess) {
            soup.release();
            if (!rc) HIPCHK_FN(e);
            return 1;
        }
        if (timer.ms(&got.kernel_ms) != hipSuccess) got.kernel_ms = 0.0;
        int64_t n[5] = {0, 0, 0, 0, 0};
        for (long long i = 0; i < nu; i++) n[codes[(size_t)i] < 5 ? codes[(size_t)i] : 0]++;
        got.left = n[0]; got.snapped = n[1]; got.held = n[2]; got.flat = n[3]; got.nan = n[4];
        if (h_status) memcpy(h_status, codes.data(), (size_t)nu);
    }
    *stats = got;
    *out = derived_mesh(m, soup, soup.p ? (int64_t)nt : 0);
    return 0;
}

// ---- support rays through the field: the true support volume per build direction ----
static thread_local double g_supports_ms[4] = {0.0, 0.0, 0.0, 0.0};

int sdf_mesh_support_rays(sdf_mesh *m, sdf_tape *t, const double *h_dirs, int64_t n_dirs, const double *params8, int max_steps, int refine,
                          sdf_support_rays **out, double *h_values, int64_t *h_counts) {
    if (out) *out = nullptr;
    if (!m || !t || !h_dirs || !params8 || !out || !h_values || !h_counts) REFUSE("NULL argument");
    if (probe_refused(__func__, m, t, false, "every step of every ray would need a host round trip")) return 2;
    for (int i = 0; i < 8; i++) if (!std::isfinite(params8[i])) REFUSE("the parameters are not finite");
    SupportParams p;
    p.sin_limit = params8[0]; p.bed_tol = params8[1]; p.start = params8[2]; p.min_step = params8[3]; p.step_scale = params8[4];
    p.max_steps = max_steps; p.refine = refine;
    if (march_refused(__func__, p.start, p.min_step, p.step_scale, INFINITY, max_steps, refine)) return 2;
    if (n_dirs > SUPPORT_MAX_DIRS) REFUSE("more than 1024 directions");
    if (overhang_refused(__func__, h_dirs, (long long)n_dirs, p.sin_limit, p.bed_tol)) return 2;
    MESH_READY(m);
    if ((long long)m->st.n_triangles >= (1ll << 31)) REFUSE("2^31 or more triangles");
    if (m->st.n_triangles > 0 && !mesh_soup(m) && !m->records) REFUSE("the mesh has no soup on the device");
    for (int k = 0; k < 4; k++) g_supports_ms[k] = 0.0;
    for (int64_t k = 0; k < n_dirs; k++) {                             // the empty result: no launch for a mesh of 0 triangles
        h_values[7 * k] = INFINITY; h_values[7 * k + 1] = -INFINITY;
        for (int c = 2; c < 7; c++) h_values[7 * k + c] = 0.0;
        for (int c = 0; c < 6; c++) h_counts[6 * k + c] = 0;
    }
    sdf_support_rays *res = new sdf_support_rays();
    struct Guard { sdf_support_rays *r; ~Guard() { delete r; } } guard{res};      // (its blocks go back with it)
    res->ctx = m->ctx;
    res->dirs.resize((size_t)n_dirs);
    if (m->st.n_triangles > 0) {
        MESH_SOUP_READY(m);
        HIPCHK(set_device(m->ctx->device));
        if (support_rays_run(m->ctx->stream, t->d_code, t->d_c64, t->full, (const double *)mesh_soup(m), (long long)m->st.n_triangles, h_dirs,
                             (long long)n_dirs, p, &res->dirs, h_values, h_counts, g_supports_ms)) return 1;
    }
    guard.r = nullptr;
    *out = res;
    return 0;
}

int sdf_support_rays_fetch(sdf_support_rays *r, int64_t k, int32_t *h_triangle, double *h_height, uint8_t *h_status, int32_t *h_steps,
                           double *h_origin) {
    if (!r) { fail("sdf_support_rays_fetch: NULL argument"); return 2; }
    if (k < 0 || k >= (int64_t)r->dirs.size()) { fail("sdf_support_rays_fetch: no such direction"); return 2; }
    const SupportRaysDir &d = r->dirs[(size_t)k];
    if (d.m < 1) return 0;                                             // nothing on the device
    sdf_ctx *c = r->ctx;
    HIPCHK_FN(set_device(c->device));
    const char *base = d.block.as<char>();
    const size_t nm = (size_t)d.m;
    if (h_origin) HIPCHK_FN(hipMemcpyAsync(h_origin, base, nm * 24, hipMemcpyDeviceToHost, c->stream));
    if (h_height) HIPCHK_FN(hipMemcpyAsync(h_height, base + d.o_height, nm * 8, hipMemcpyDeviceToHost, c->stream));
    if (h_triangle) HIPCHK_FN(hipMemcpyAsync(h_triangle, base + d.o_triangle, nm * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_steps) HIPCHK_FN(hipMemcpyAsync(h_steps, base + d.o_steps, nm * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_status) HIPCHK_FN(hipMemcpyAsync(h_status, base + d.o_status, nm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_FN(stream_wait(c->stream));
    return 0;
}

int sdf_support_rays_destroy(sdf_support_rays *r) {
    if (!r) return 0;
    (void)hipSetDevice(r->ctx->device);
    delete r;
    return 0;
}

double sdf_mesh_supports_last_kernel_ms(double *parts4) {
    for (int k = 0; parts4 && k < 4; k++) parts4[k] = g_supports_ms[k];
    return g_supports_ms[0] + g_supports_ms[1] + g_supports_ms[2] + g_supports_ms[3];
}

// ---- sphere tracing of a model: depth, normal, steps and status per pixel ----
static thread_local double g_render_kernel_ms = 0.0;

// One device allocation, freed before it returns; sdf_render_last_kernel_ms: the kernel alone, by HIP events on the context's stream.
int sdf_render_host(sdf_tape *t, const double *frame18, int width, int height, const double *params5, int max_steps, int refine,
                    double *h_depth, double *h_normal, int32_t *h_steps, uint8_t *h_status) {
    if (!t) REFUSE("NULL argument");
    if (t->n_extern) REFUSE("the tape reads user closures (L_EXTERN): every step of every ray would need a host round trip");
    HIPCHK(set_device(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    if (!t->d_code || !t->d_c64 || !frame18 || !params5 || !h_depth || !h_normal || !h_steps || !h_status) REFUSE("NULL argument");
    if (width < 1 || height < 1) REFUSE("empty image: " + std::to_string(width) + " x " + std::to_string(height));
    if ((long long)width * height > (1ll << 26)) REFUSE("image of " + std::to_string(width) + " x " + std::to_string(height) + ": more than 2^26 pixels");
    if (max_steps < 1) REFUSE("max_steps must be at least 1");
    if (refine < 0) REFUSE("refine must not be negative");
    for (int i = 0; i < 18; i++) if (!std::isfinite(frame18[i])) REFUSE("the ray frame is not finite");
    for (int i = 0; i < 5; i++) if (!std::isfinite(params5[i])) REFUSE("the march parameters are not finite");
    const double t_near = params5[0], t_far = params5[1], hit_eps = params5[2], step_scale = params5[3], normal_eps = params5[4];
    if (!(hit_eps > 0.0)) REFUSE("hit_eps must be positive");
    if (!(normal_eps > 0.0)) REFUSE("normal_eps must be positive");
    if (!(step_scale > 0.0 && step_scale <= 1.0)) REFUSE("step_scale must lie in (0, 1]");
    if (t_far < t_near) REFUSE("t_far lies before t_near");

    RenderArgs a;
    for (int i = 0; i < 3; i++) {
        a.o0[i] = frame18[i]; a.ou[i] = frame18[3 + i]; a.ov[i] = frame18[6 + i];
        a.c[i] = frame18[9 + i]; a.du[i] = frame18[12 + i]; a.dv[i] = frame18[15 + i];
    }
    a.t_near = t_near; a.t_far = t_far; a.hit_eps = hit_eps; a.step_scale = step_scale; a.normal_eps = normal_eps;
    a.width = width; a.height = height; a.max_steps = max_steps; a.refine = refine;
    a.tiles_x = (width + 7) / 8;
    a.n_tiles = a.tiles_x * ((height + 7) / 8);                        // (at most 2^26 pixels: below 2^27 tiles even for a one-pixel-wide image)
    const size_t n = (size_t)width * (size_t)height;
    double *depth, *normal;
    int32_t *steps;
    uint8_t *status;
    Scratch scratch(st);
    scratch.part(&depth, n); scratch.part(&normal, 3 * n); scratch.part(&steps, n); scratch.part(&status, n);
    EventTimer timer;
    HIPCHK_FN(scratch.alloc());
    TIMED_LAUNCH(st, HIPCHK_MSG("sdf_render_host: hipGetLastError(): ", (hipError_t)launch_render(st, t->d_code, t->d_c64, t->full, a, depth, normal, steps, status)));
    HIPCHK_FN(hipMemcpyAsync(h_depth, depth, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_normal, normal, n * 24, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_steps, steps, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK_FN(hipMemcpyAsync(h_status, status, n, hipMemcpyDeviceToHost, st));
    TIMED_RESULTS(st, &g_render_kernel_ms);
    return 0;
}

double sdf_render_last_kernel_ms(void) { return g_render_kernel_ms; }

}  // extern "C"
