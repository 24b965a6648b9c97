// sdf_probe.h -- what the field probes share on the device: k_vertex_normals, k_vertex_thickness, k_support_rays,
// k_triangle_deviation, k_vertex_snap and k_render each inline the tape interpreter and evaluate the field around a mesh or an image.
//
// The doctrine of a probe kernel.  The interpreter is inlined ONCE: everything a lane evaluates -- the passes of a gradient, the steps
// of a march, the halvings of a bisection -- is a pass of ONE loop around the one run_tape1, and the loop's phase and counter are
// wave-uniform (a phase ends after a fixed number of passes or when `__any(...)` says no lane has work in it).  Lanes never branch
// around the interpreter: the probes' units are built with the structurizer option that is only safe for wave-uniform control flow
// (build.units).  A lane takes its state changes by selects; one that is done keeps evaluating at its frozen point and discards the
// value; one beyond the last item evaluates the last item and stores nothing; a wave that lies wholly beyond it leaves (wave-uniform).
// A kernel's own head says only what is its own: its phases, its states, what a dead lane evaluates.
//
// The pieces below take and return VALUES; the five lines that give a lane its item stay in the kernels, and so does a use of a
// piece through which a kernel does not keep its instructions: profiles/probe_spine_refactor.md has the reasons.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfk {

// The central difference, six passes k = 0 .. 5 of the kernel's loop: pass k evaluates at p moved along axis k / 2, by + eps when k
// is even and by + (-eps) when it is odd, and the odd passes leave value(+) - value(-) in g0 / g1 / g2.
struct P3 { double x, y, z; };
__device__ __forceinline__ P3 grad_point(int k, double eps, double px, double py, double pz) {
    const double h = (k & 1) ? -eps : eps;
    P3 p = {px, py, pz};
    if ((k >> 1) == 0) p.x = p.x + h;
    else if ((k >> 1) == 1) p.y = p.y + h;
    else p.z = p.z + h;
    return p;
}

struct Grad { double gp, g0, g1, g2; };                                // the previous pass's value, the three differences
__device__ __forceinline__ Grad grad_take(Grad g, int k, double v) {
    const double d = g.gp - v;
    if (k == 1) g.g0 = d;
    else if (k == 3) g.g1 = d;
    else if (k == 5) g.g2 = d;
    g.gp = v;
    return g;
}

// |g|^2 in the definitions' order, and the test of a length (or a squared length) that gives no direction: 0 or NaN
__device__ __forceinline__ double grad_len2(double g0, double g1, double g2) { return (g0 * g0 + g1 * g1) + g2 * g2; }
__device__ __forceinline__ bool grad_flat(double len) { return len == 0.0 || len != len; }

}  // namespace sdfk
