// sdf_contour.h -- the case table of the contouring kernels (sdf_contour.hip), the same data as CASES of
// tests/contour_ref.py (tests/test_contour_host.py compares the two).  Cell (ix, iy) has the corners c0 = V[ix][iy], c1 = V[ix + 1][iy],
// c2 = V[ix + 1][iy + 1], c3 = V[ix][iy + 1] and the edges 0 bottom (c0 c1), 1 right (c1 c2), 2 top (c2 c3), 3 left (c3 c0); its case is
// the sum of 1 << k over its inside corners (v < level).  A row is {segments, from0, to0, from1, to1}: a segment runs from edge to
// edge with the inside on its left.  The saddles 5 and 10 are listed for a centre value that is inside; a centre that is outside
// swaps their two `to` edges.
#pragma once
#include <hip/hip_runtime.h>

__constant__ static const unsigned char CONTOUR_CASES[16][5] = {
    {0, 0, 0, 0, 0},
    {1, 0, 3, 0, 0},
    {1, 1, 0, 0, 0},
    {1, 1, 3, 0, 0},
    {1, 2, 1, 0, 0},
    {2, 0, 1, 2, 3},
    {1, 2, 0, 0, 0},
    {1, 2, 3, 0, 0},
    {1, 3, 2, 0, 0},
    {1, 0, 2, 0, 0},
    {2, 1, 2, 3, 0},
    {1, 1, 2, 0, 0},
    {1, 3, 1, 0, 0},
    {1, 0, 1, 0, 0},
    {1, 3, 0, 0, 0},
    {0, 0, 0, 0, 0},
};
