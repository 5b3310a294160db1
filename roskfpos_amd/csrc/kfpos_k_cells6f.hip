/*
 * kfpos_k_cells6f.hip -- k_step_toa6 around CellArgs, full covariance layout: banks with anchor cells and ML initialisation
 */
#include "kfpos_kernels.h"

namespace {

#include "kfpos_k_toa6.inc"

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::cells_kernel_t cells_toa6_full(int as, int heur) { return cells_toa6_kernel<false, REAL, MREAL>(as, heur); }
kfpos_k::cells_kernel_t kfpos_k::cells_toa6_full_kernel(int st, int as, int heur) {
    return KFPOS_BY_STORAGE(st, cells_toa6_full, as, heur);
}
