// sdf_components.h -- the connected shells of a welded mesh on the device (sdf_components.hip): labelling,
// numbering, counts and boxes, and the compaction that turns "these shells" into a soup of its own.  Both calls are synchronous on
// `st`, take their scratch in one hooked allocation that is back when they return, and return 0, or 1 with the message set.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdf_hip.h"
#include "sdf_runtime.h"
namespace sdfk {
// what a labelled mesh keeps, one device block: [vertex_shell V x i32 | triangle_shell T x i32 | triangles K x u64 | vertices K x u64 |
// box K x 6 keys of box_key (sdf_block.h): lo x, y, z, hi x, y, z], every part 256-byte aligned
struct ShellParts {
    int *vertex_shell, *triangle_shell;
    unsigned long long *triangles, *vertices, *box;
};
size_t shell_block_bytes(long long n_vertices, long long n_tris, long long n_shells);
ShellParts shell_parts(void *block, long long n_vertices, long long n_tris, long long n_shells);
// d_cells: n_tris x 3 int64 indices below n_vertices, d_points: n_vertices x 3 float64 (the weld's; 1 <= n_tris, n_vertices < 2^31).
// On success *block holds the device block laid out as above for *n_shells shells (a failed call leaves it empty); *rounds: the hook passes
// run, the verifying one included; kernel_ms[0]: labelling (with the host's look at the counter between the rounds), kernel_ms[1]:
// numbering, counts and boxes, by HIP events
int components_label(hipStream_t st, const long long *d_cells, const double *d_points, long long n_tris, long long n_vertices,
                     DevBlock *block, long long *n_shells, int *rounds, double kernel_ms[2]);
// the triangles of d_soup (n_tris x 9 float64) whose shell k has h_keep[k] != 0, in soup order, into `out` (grown as needed; left
// alone when nothing is kept); *n_kept: how many
int components_select(hipStream_t st, const double *d_soup, long long n_tris, const int *d_triangle_shell, const unsigned char *h_keep,
                      long long n_shells, DevBuf *out, long long *n_kept, double *kernel_ms);
// the copy of every compaction of a soup (a selection's, a mended mesh's): the nine doubles of every triangle of d_soup (n_tris x 9
// float64) whose flag is set go to d_out + 9 * d_pos[triangle], one lane per double of the source; returns the launch's error
hipError_t select_copy(hipStream_t st, const double *d_soup, const int *d_flags, const int *d_pos, long long n_tris, void *d_out);
// box keys -> float64 on the host (h_bounds: n_shells x 2 x 3)
void shell_bounds(const unsigned long long *h_keys, long long n_shells, double *h_bounds);
}
