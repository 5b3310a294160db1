/*
 * kfpos_k_imu9.hip -- k_step_imu9 around KArgs: the 9-state UWB + IMU step (kfpos_k_imu9.inc), the bench kernel
 */
#include "kfpos_kernels.h"

namespace {

#include "kfpos_k_imu9.inc"

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::step_kernel_t imu9_of(int as, bool ranging) {
    if (!ranging) return k_step_imu9<REAL, MREAL, 0, false>; /* no epoch: the anchor count plays no role */
    if (as == 8) return k_step_imu9<REAL, MREAL, 8>;
    return k_step_imu9<REAL, MREAL, 0>;
}
kfpos_k::step_kernel_t kfpos_k::imu9_kernel(int st, int as, bool ranging) {
    return KFPOS_BY_STORAGE(st, imu9_of, as, ranging);
}
