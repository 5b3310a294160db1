/*
 * kfpos_k_tags.hip -- per-tag lifecycle kernels (kfpos_get_tags / kfpos_set_tags / kfpos_reset_tags): read, write or
 * re-initialise the filters of a LIST of tags, at a cost that follows the length of the list and not the size of the bank;
 * and the gather / scatter between the bank and the compact work bank on which a row-list step (kfpos_step_*_rows,
 * kfpos_slot_submit_rows) runs the unchanged step kernels (k_rows_work, below).
 *
 * Work item = one (listed tag, component). The staging side is row-major per listed tag, section after section
 * (x | P | latch | height, the formats of kfpos_get_state / kfpos_get_latch / kfpos_get_height), and work item g reads
 * or writes staging element g: consecutive lanes touch consecutive 8-byte words. The bank side is a gather / scatter at
 * stride T, one element per work item -- unavoidable with a component-major bank, and the list is short against T.
 *
 * Where a component lives (which array, which row, which element type) is not written down here: the host hands the
 * kernels a table (TagArgs::comp) from kfpos_state_record.h, the very table the whole-bank accessors walk on the CPU
 * (kfpos_hip_state.hip: bank_transfer); elements are decoded and encoded through ldrow / strow / ldcov / stcov.
 * Row indices are validated on the host before any launch: no kernel sees a row outside [0, T).
 */
#include "kfpos_stored.h"

namespace {

using kfpos_k::TagArgs;
using kfpos_k::TagComp;

/* work item g -> (listed tag i, component c of the record); false when g lies beyond the last section */
__device__ inline bool tag_item(const TagArgs &a, size_t g, uint32_t &i, int &c) {
    size_t r = g;
#pragma unroll
    for (int s = 0; s < kfpos_k::TAG_SECTIONS; ++s) {
        const size_t cnt = (size_t)a.n * a.w[s];
        if (r < cnt) {
            i = (uint32_t)(r / a.w[s]);
            c = a.cbase[s] + (int)(r % a.w[s]);
            return true;
        }
        r -= cnt;
    }
    return false;
}

template <typename REAL, typename MREAL>
__global__ __launch_bounds__(256) void k_tags_gather(const TagArgs a) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a.fl && g < (size_t)a.n) a.fl[g] = a.flags[a.rows[g]];
    uint32_t i;
    int c;
    if (!tag_item(a, g, i, c)) return;
    const uint32_t t = (uint32_t)a.rows[i];
    const TagComp d = a.comp[c];
    const size_t T = a.T;
    double v = 0.0; /* TC_NONE: a component the model does not store (a = 0 of the 9-state x, the planar ax ay) */
    if (d.kind == kfpos_k::TC_F64) v = ldrow<double>(a.buf[d.buf], d.row, T, t);
    else if (d.kind == kfpos_k::TC_COV) v = ldcov<REAL>(a.buf[d.buf], d.row, a.psz, T, t);
    else if (d.kind == kfpos_k::TC_REAL) v = ldrow<MREAL>(a.buf[d.buf], d.row, T, t);
    a.val[g] = v;
}

template <typename REAL, typename MREAL>
__global__ __launch_bounds__(256) void k_tags_scatter(const TagArgs a) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a.fl && g < (size_t)a.n) a.flags[a.rows[g]] = a.fl[g];
    uint32_t i;
    int c;
    if (!tag_item(a, g, i, c)) return;
    const TagComp d = a.comp[c];
    if (!d.aux) return; /* not stored, or the mirror image of a stored entry (symmetric layouts keep j >= i) */
    const uint32_t t = (uint32_t)a.rows[i];
    const size_t T = a.T;
    const double v = a.val[g];
    if (d.kind == kfpos_k::TC_F64) strow<double>(a.buf[d.buf], d.row, T, t, v);
    else if (d.kind == kfpos_k::TC_COV) stcov<REAL>(a.buf[d.buf], d.row, a.psz, T, t, v);
    else if (d.kind == kfpos_k::TC_REAL) strow<MREAL>(a.buf[d.buf], d.row, T, t, v);
}

/* comp[] lists the STORED rows of a tag here (n_comp of them); aux says what a fresh handle holds there: 0 = zero
 * (which every storage mode encodes as zero words), 1..3 = x y z of the start position, 4 / 5 = the planar filter's
 * height / angle */
template <typename REAL, typename MREAL>
__global__ __launch_bounds__(256) void k_tags_reset(const TagArgs a) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < (size_t)a.n) a.flags[a.rows[g]] = 0u;
    if (g >= (size_t)a.n * a.n_comp) return;
    const uint32_t i = (uint32_t)(g / a.n_comp);
    const TagComp d = a.comp[g % a.n_comp];
    const uint32_t t = (uint32_t)a.rows[i];
    const size_t T = a.T;
    double v = 0.0;
    if (d.aux >= 1 && d.aux <= 3 && a.init) v = a.init[(size_t)i * 3 + (d.aux - 1)];
    else if (d.aux) v = a.cst[d.aux - 1];
    if (d.kind == kfpos_k::TC_F64) strow<double>(a.buf[d.buf], d.row, T, t, v);
    else if (d.kind == kfpos_k::TC_COV) stcov<REAL>(a.buf[d.buf], d.row, a.psz, T, t, v);
    else if (d.kind == kfpos_k::TC_REAL) strow<MREAL>(a.buf[d.buf], d.row, T, t, v);
}

/* ---- the work bank of a row-list step: stored bits of the listed tags, bank <-> work, no decode ----
 * Grid: x = 256 listed tags (tag index fastest: the work side, stride n, is fully coalesced), y = stored row of
 * comp[] (block-uniform), the last y = the flags word. The bank side is one scattered 2-8 byte access per item. */
template <typename E, bool TO_BANK>
__device__ inline void raw_move(void *bank, void *work, size_t row, size_t T, size_t n, uint32_t t, uint32_t i) {
    E *b = ((E *)bank) + row * T, *w = ((E *)work) + row * n;
    if (TO_BANK) b[t] = w[i];
    else w[i] = b[t];
}
template <typename REAL, typename MREAL, bool TO_BANK>
__global__ __launch_bounds__(256) void k_rows_work(const TagArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const uint32_t t = (uint32_t)a.rows[i];
    const size_t T = a.T, n = a.n;
    const int c = blockIdx.y;
    if (c == a.n_comp) {
        raw_move<uint32_t, TO_BANK>(a.flags, a.wflags, 0, T, n, t, i);
        return;
    }
    const TagComp d = a.comp[c];
    void *bank = a.buf[d.buf], *work = a.wbuf[d.buf];
    using RAWM = std::conditional_t<sizeof(MREAL) == 4, uint32_t, uint64_t>;
    if (d.kind == kfpos_k::TC_F64) raw_move<uint64_t, TO_BANK>(bank, work, d.row, T, n, t, i);
    else if (d.kind == kfpos_k::TC_REAL) raw_move<RAWM, TO_BANK>(bank, work, d.row, T, n, t, i);
    else if (d.kind == kfpos_k::TC_COV) {
        if constexpr (std::is_same<REAL, p48>::value) { /* both planes: [psz][.] uint32, then [psz][.] uint16 */
            raw_move<uint32_t, TO_BANK>(bank, work, d.row, T, n, t, i);
            raw_move<uint16_t, TO_BANK>(((uint32_t *)bank) + (size_t)a.psz * T, ((uint32_t *)work) + (size_t)a.psz * n,
                                        d.row, T, n, t, i);
        } else {
            using RAWC = std::conditional_t<sizeof(REAL) == 4, uint32_t, uint64_t>;
            raw_move<RAWC, TO_BANK>(bank, work, d.row, T, n, t, i);
        }
    }
}

template <typename REAL, typename MREAL>
void launch_tags_as(int op, int blocks, hipStream_t s, const TagArgs &a) {
    if (op == kfpos_k::TAGS_WORK_IN || op == kfpos_k::TAGS_WORK_OUT) {
        const dim3 grid((a.n + 255) / 256, a.n_comp + 1);
        if (op == kfpos_k::TAGS_WORK_IN) hipLaunchKernelGGL((k_rows_work<REAL, MREAL, false>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_rows_work<REAL, MREAL, true>), grid, dim3(256), 0, s, a);
        return;
    }
    if (op == kfpos_k::TAGS_GATHER) hipLaunchKernelGGL((k_tags_gather<REAL, MREAL>), dim3(blocks), dim3(256), 0, s, a);
    else if (op == kfpos_k::TAGS_SCATTER) hipLaunchKernelGGL((k_tags_scatter<REAL, MREAL>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_tags_reset<REAL, MREAL>), dim3(blocks), dim3(256), 0, s, a);
}

} // namespace

void kfpos_k::launch_tags(int op, int st, hipStream_t s, const TagArgs &a) {
    size_t items = a.n;
    if (op == TAGS_RESET || op == TAGS_WORK_IN || op == TAGS_WORK_OUT) {
        if ((size_t)a.n * a.n_comp > items) items = (size_t)a.n * a.n_comp;
    } else {
        size_t w = 0;
        for (int k = 0; k < TAG_SECTIONS; ++k) w += a.w[k];
        if ((size_t)a.n * w > items) items = (size_t)a.n * w;
    }
    if (items == 0) return;
    const int blocks = (int)((items + 255) / 256);
    KFPOS_BY_STORAGE(st, launch_tags_as, op, blocks, s, a);
}
