/*
 * kfpos_k_cells9.hip -- k_step_imu9 around CellArgs (kfpos_k_imu9.inc): the 9-state UWB + IMU ranging round (MODE_TOA,
 * MODE_FUSED) of a bank with anchor cells (kfpos_set_anchor_cells). IMU-only rounds read no anchor and stay with the
 * kernel of kfpos_k_imu9.hip: RANGING = false is not built here.
 */
#include "kfpos_kernels.h"

namespace {

#include "kfpos_k_imu9.inc"

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::cells_kernel_t cells_imu9_of(int as) {
    if (as == 8) return k_step_imu9<REAL, MREAL, 8, true, CellArgs>;
    return k_step_imu9<REAL, MREAL, 0, true, CellArgs>;
}
kfpos_k::cells_kernel_t kfpos_k::cells_imu9_kernel(int st, int as) { return KFPOS_BY_STORAGE(st, cells_imu9_of, as); }
