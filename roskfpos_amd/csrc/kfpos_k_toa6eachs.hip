/*
 * kfpos_k_toa6eachs.hip -- k_trace_toa6_each, symmetric (packed) covariance layout: banks with a fixed start
 */
#include "kfpos_kernels.h"

namespace {

#include "kfpos_k_toa6each.inc"

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::trace_each_kernel_t toa6_each_sym(int as, int heur) { return toa6_each_kernel<true, REAL, MREAL>(as, heur); }
kfpos_k::trace_each_kernel_t kfpos_k::toa6_each_sym_kernel(int st, int as, int heur) {
    return KFPOS_BY_STORAGE(st, toa6_each_sym, as, heur);
}
