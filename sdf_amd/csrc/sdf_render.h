// sdf_render.h -- host entry of the sphere tracer (sdf_render.hip, k_render): 0 done, 1 HIP error, 2 refused before any allocation or
// launch; `err` says why.  d_code / d_consts: a float64 tape on the device; full: it uses the trigonometric ops.  One device allocation,
// freed before it returns; *kernel_ms (may be NULL): the kernel alone, by HIP events on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
namespace sdfk {
int render_host(hipStream_t st, const uint32_t *d_code, const double *d_consts, bool full, const double *frame18, int width, int height,
                const double *params5, int max_steps, int refine, double *h_depth, double *h_normal, int32_t *h_steps, uint8_t *h_status,
                double *kernel_ms, std::string &err);
}
