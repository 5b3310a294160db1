/*
 * kfpos_k_cells6s.hip -- k_step_toa6 around CellArgs, symmetric (packed) covariance layout: banks with anchor cells and a fixed start
 */
#include "kfpos_kernels.h"

namespace {

#include "kfpos_k_toa6.inc"

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::cells_kernel_t cells_toa6_sym(int as, int heur) { return cells_toa6_kernel<true, REAL, MREAL>(as, heur); }
kfpos_k::cells_kernel_t kfpos_k::cells_toa6_sym_kernel(int st, int as, int heur) {
    return KFPOS_BY_STORAGE(st, cells_toa6_sym, as, heur);
}
