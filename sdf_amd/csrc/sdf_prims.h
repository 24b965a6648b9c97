// sdf_prims.h -- numbering flagged items, the step every compaction of the mesh readers shares (sdf_prims.hip; the roots and the kept
// triangles of sdf_components.hip, the clusters and the live triangles of sdf_simplify.hip, the survivors of sdf_mend.hip).  The library's int scan (hipCUB) is
// instantiated there, once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace sdfk {
// raises *bytes to what the exclusive scan of n flags needs as temporary storage, and to 1 at the least: a unit that also sorts
// puts the sizes of its sorts into *bytes first and sizes one `tmp` part for all of them
hipError_t scan_tmp_bytes(hipStream_t st, long long n, size_t *bytes);
// pos[i] = the number of set flags before i (1 <= n < 2^31; tmp: tmp_bytes as scan_tmp_bytes said for n or more), *count = how
// many are set: the last position + the last flag, read back behind ONE wait for the stream -- a copy the caller enqueued before
// the call has landed too.  Returns 0, or 1 with the message set: a HIP error, or "<who>the scan of the <what> is inconsistent"
// for a count outside 0 .. n
int number_flags(const char *who, const char *what, hipStream_t st, int *flags, int *pos, long long n, void *tmp, size_t tmp_bytes,
                 long long *count);
// the same for items that each count 0 or more (the segments of a cell, the points of a contour: sdf_contour.hip): pos[i] = the sum of
// the counts before i, *total = the sum of all of them, which the caller bounds by max_total < 2^31 -- "<who>the scan of the <what> is
// inconsistent" for a total outside 0 .. max_total.  number_flags is this with max_total = n
int number_counts(const char *who, const char *what, hipStream_t st, int *counts, int *pos, long long n, long long max_total, void *tmp,
                  size_t tmp_bytes, long long *total);
// the bits that hold 0 .. n - 1: where a library radix sort over such keys may stop
static inline int bits_for(long long n) { int b = 1; while (b < 63 && (1ll << b) < n) b += 1; return b; }
}
