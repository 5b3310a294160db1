/*
 * kfpos_k_toa6eachf.hip -- k_trace_toa6_each, full 6x6 covariance layout: banks that start with the ML initialisation (non-symmetric P)
 */
#include "kfpos_kernels.h"

namespace {

#include "kfpos_k_toa6each.inc"

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::trace_each_kernel_t toa6_each_full(int as, int heur) { return toa6_each_kernel<false, REAL, MREAL>(as, heur); }
kfpos_k::trace_each_kernel_t kfpos_k::toa6_each_full_kernel(int st, int as, int heur) {
    return KFPOS_BY_STORAGE(st, toa6_each_full, as, heur);
}
