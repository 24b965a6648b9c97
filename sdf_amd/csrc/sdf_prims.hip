// sdf_prims.hip -- the one definition of sdf_prims.h: the library exclusive scan over int flags (rocPRIM through hipCUB, like the
// weld's sort) and the count it ends on.  No floating point and no kernel of its own; built with the plain flags, like sdf_weld.hip.
#include "sdf_prims.h"

#include <hipcub/hipcub.hpp>

#include <string>

#include "sdf_runtime.h"

namespace sdfk {

hipError_t scan_tmp_bytes(hipStream_t st, long long n, size_t *bytes) {
    size_t need = 0;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, (int *)nullptr, (int *)nullptr, (int)n, st);
    if (need > *bytes) *bytes = need;
    if (*bytes < 1) *bytes = 1;
    return e;
}

int number_counts(const char *who, const char *what, hipStream_t st, int *counts, int *pos, long long n, long long max_total, void *tmp,
                  size_t tmp_bytes, long long *count) {
    int h_last[2] = {0, 0};                                            // the last item: its position, its count
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, counts, pos, (int)n, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_last[0], pos + (n - 1), 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_last[1], counts + (n - 1), 4, hipMemcpyDeviceToHost, st);
    const hipError_t waited = stream_wait(st);                         // (before `h_last` goes, whatever the copies said)
    HIPCHK_MSG(who, e);
    HIPCHK_MSG(who, waited);
    *count = (long long)h_last[0] + h_last[1];
    if (*count < 0 || *count > max_total) return fail(std::string(who) + "the scan of the " + what + " is inconsistent");
    return 0;
}

int number_flags(const char *who, const char *what, hipStream_t st, int *flags, int *pos, long long n, void *tmp, size_t tmp_bytes,
                 long long *count) {
    return number_counts(who, what, st, flags, pos, n, n, tmp, tmp_bytes, count);
}

}  // namespace sdfk
