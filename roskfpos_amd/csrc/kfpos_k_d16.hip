/*
 * kfpos_k_d16.hip -- k_decode_d16: the device side of KFPOS_SLOT_RANGES_D16 (kfpos.h, kfpos_d16.h). A round's int16 codes
 * and its escape list become the int32 range matrix the unchanged step kernels read, and the device base moves with it.
 * The text it is judged against is kfpos_d16_decode_ref (kfpos_d16.h).
 *
 * One pass over the flat matrix, memory-bound: per element 2 bytes of code and 4 of base in, 4 + 4 bytes out. Work item g
 * below ceil(n / 8) owns elements 8 g ... 8 g + 7: one 16-byte load of codes, two 16-byte loads of base, two 16-byte
 * stores each of ranges and base -- the matrix is addressed flat, so a vector may straddle two anchor rows, and n_tags
 * need be a multiple of nothing; the last item takes what is left one element at a time. The work items behind those
 * apply one escape entry each. An ESCAPE-coded element is written by its escape entry alone: an item that finds one among
 * its eight codes stores the other seven one by one (rare: a first appearance, an NLOS jump), so the order of the two kinds
 * of item does not matter. With a per-tag dt (KFPOS_SLOT_DT_PER_TAG) the tag of element e is e % n_tags; the codes and
 * entries of a tag whose dt < 0 are not used: it decodes to 0 and keeps its base.
 * Indices are validated on the host before the launch (kfpos_hip_slots.hip: d16_check); no item touches an element
 * outside [0, n) whatever the list holds.
 */
#include "kfpos_kargs.h"

namespace {

using kfpos_k::D16Args;

typedef short short8 __attribute__((ext_vector_type(8)));
constexpr uint32_t D16_VEC = 8;

__device__ inline int32_t d16_sum(int32_t base, int32_t code) { return (int32_t)((uint32_t)base + (uint32_t)code); }

__global__ __launch_bounds__(256) void k_decode_d16(const D16Args a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nvec = (a.n + D16_VEC - 1) / D16_VEC;
    if (g >= nvec) { /* an escape entry */
        const uint32_t k = g - nvec;
        if (k >= a.n_esc) return;
        const int2 p = ((const int2 *)a.esc)[k];
        const uint32_t e = (uint32_t)p.x;
        if (e >= a.n) return;
        if (a.dt && a.dt[e % a.T] < 0.0) return;
        a.out[e] = p.y;
        a.base[e] = p.y;
        return;
    }
    const uint32_t e0 = g * D16_VEC;
    uint32_t t = a.dt ? e0 % a.T : 0u;
    if (e0 + D16_VEC <= a.n) {
        const short8 c = *(const short8 *)(a.code + e0);
        int4 *bp = (int4 *)(a.base + e0), *op = (int4 *)(a.out + e0);
        const int4 b0 = bp[0], b1 = bp[1];
        int32_t b[D16_VEC] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w}, o[D16_VEC];
        uint32_t escaped = 0u;
#pragma unroll
        for (uint32_t j = 0; j < D16_VEC; ++j) {
            bool skip = false;
            if (a.dt) {
                skip = a.dt[t] < 0.0;
                if (++t == a.T) t = 0u;
            }
            const int32_t cj = c[j];
            o[j] = 0;
            if (skip || cj == KFPOS_D16_ABSENT) continue;
            if (cj == KFPOS_D16_ESCAPE) escaped |= 1u << j;
            else o[j] = b[j] = d16_sum(b[j], cj);
        }
        if (escaped == 0u) {
            op[0] = make_int4(o[0], o[1], o[2], o[3]);
            op[1] = make_int4(o[4], o[5], o[6], o[7]);
            bp[0] = make_int4(b[0], b[1], b[2], b[3]);
            bp[1] = make_int4(b[4], b[5], b[6], b[7]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < D16_VEC; ++j)
                if (!(escaped >> j & 1u)) {
                    a.out[e0 + j] = o[j];
                    a.base[e0 + j] = b[j];
                }
        }
        return;
    }
    for (uint32_t e = e0; e < a.n; ++e) { /* the tail */
        bool skip = false;
        if (a.dt) {
            skip = a.dt[t] < 0.0;
            if (++t == a.T) t = 0u;
        }
        const int32_t ce = a.code[e];
        if (skip || ce == KFPOS_D16_ABSENT) a.out[e] = 0;
        else if (ce != KFPOS_D16_ESCAPE) a.out[e] = a.base[e] = d16_sum(a.base[e], ce);
    }
}

} // namespace

void kfpos_k::launch_decode_d16(hipStream_t s, const D16Args &a) {
    if (a.n == 0) return;
    const uint32_t items = (a.n + D16_VEC - 1) / D16_VEC + a.n_esc; /* n, n_esc <= INT32_MAX: no wrap */
    hipLaunchKernelGGL(k_decode_d16, dim3((items + 255u) / 256u), dim3(256), 0, s, a);
}
