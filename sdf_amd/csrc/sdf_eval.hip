// sdf_eval.hip -- f(P) alone: the tape interpreter over caller-supplied points (k_eval_points, with user closures k_eval_points_ext),
// over a grid given by its axes (k_eval_grid) and over the tiles of a chunk of batches (k_eval_tiles, enqueue_eval_tiles: what
// sdf_chunked.hip samples with for batch_size > 32), and the entry points of the C ABI that evaluate a tape without meshing it --
// sdf_eval_*, the two *_extern_* phases, sdf_estimate_bounds (its kernel k_estimate_bounds lives in sdf_bounds.hip).
//
// Every kernel here IS the interpreter and nothing else: one bounds test per lane, then run_tape1, whose branches are all wave-uniform
// and whose dispatch is a scalar jump through a table (sdf_interp.h).  So the unit takes the interpreters' flags, WITH the structurizer
// option (build.units); the prepass kernels, which also hold the interval interpreters, are sdf_prepass.hip.
#include <hip/hip_runtime.h>

#include <cstring>

#include "sdf_plain.h"
#include "sdf_bounds.h"
#include "sdf_internal.h"

using namespace sdfk;

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

// dispatch over (precision, FULL), on the context's stream (LAUNCH_TAPE_ON: sdf_interp.h)
#define LAUNCH_TAPE(KERNEL, grid, block, shmem, t, precision, ...) \
    LAUNCH_TAPE_ON((t)->ctx->stream, KERNEL, grid, block, shmem, t, precision, __VA_ARGS__)

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

}  // extern "C"

// k_eval_tiles for the nt tiles of a chunk (sdf_chunked.hip), the largest of largest_tile samples, enqueued on `st`: the axes, the
// tile table and the tiles' first samples `d_org` are on the device already; the caller checks the launch with the next ones
void enqueue_eval_tiles(sdf_tape *t, int precision, const double *dX, const double *dY, const double *dZ, const FieldTile *d_tiles,
                        const int *d_org, float *d_vol, size_t largest_tile, int nt, hipStream_t st) {
    LAUNCH_TAPE_ON(st, k_eval_tiles, dim3((unsigned)((largest_tile + 255) / 256), (unsigned)nt), dim3(256), 0, t, precision, dX, dY, dZ,
                   d_tiles, d_org, d_vol);
}
