// sdf_dual.h -- the system that places the vertex of a dual-contouring cell (sdf_dual.hip): (A + reg w I) y = b - A m by cofactors over
// the determinant, x = m + y, every line one float64 operation in the order of tests/dual_ref.py `solve`, which is that of
// tests/simplify_ref.py `solve` (the including unit is built with -ffp-contract=off).  The lines are a copy of k_cluster_vertex's
// (sdf_simplify.hip), which keeps its own between its two item walks: what follows the solve differs -- there the mean outside the
// cell, here the clamp -- and a shared function would have moved that kernel's code object for no gain.
#pragma once
#include <hip/hip_runtime.h>

namespace sdfk {

// q: A00, A01, A02, A11, A12, A22, b0, b1, b2; m: the mean about the cell's centre; x: out.  Returns w, the trace of A
__device__ __forceinline__ double quadric_solve(const double (&q)[9], const double (&m)[3], double reg, double (&x)[3]) {
    const double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5], b0 = q[6], b1 = q[7], b2 = q[8];
    const double m0 = m[0], m1 = m[1], m2 = m[2];
    const double w = (a00 + a11) + a22;
    const double lam = reg * w;
    const double g0 = b0 - ((a00 * m0 + a01 * m1) + a02 * m2);
    const double g1 = b1 - ((a01 * m0 + a11 * m1) + a12 * m2);
    const double g2 = b2 - ((a02 * m0 + a12 * m1) + a22 * m2);
    const double d00 = a00 + lam;
    const double d11 = a11 + lam;
    const double d22 = a22 + lam;
    const double c00 = (d11 * d22) - (a12 * a12);
    const double c01 = (a02 * a12) - (a01 * d22);
    const double c02 = (a01 * a12) - (a02 * d11);
    const double c11 = (d00 * d22) - (a02 * a02);
    const double c12 = (a01 * a02) - (d00 * a12);
    const double c22 = (d00 * d11) - (a01 * a01);
    const double det = (d00 * c00 + a01 * c01) + a02 * c02;
    const double y0 = ((c00 * g0 + c01 * g1) + c02 * g2) / det;
    const double y1 = ((c01 * g0 + c11 * g1) + c12 * g2) / det;
    const double y2 = ((c02 * g0 + c12 * g1) + c22 * g2) / det;
    x[0] = m0 + y0;
    x[1] = m1 + y1;
    x[2] = m2 + y2;
    return w;
}

}  // namespace sdfk
