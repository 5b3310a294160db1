/*
 * kfpos_d16.h -- the wire format of KFPOS_SLOT_RANGES_D16 (kfpos.h, "streaming slots: ranges as 16-bit deltas"): the
 * codes, the slot a producer writes them into, the encoder and a plain host decoder. C99 and C++, <stdint.h> only.
 *
 * One int16 code per element of the [max_anchors][n_tags] range matrix, flat index e = a * n_tags + t:
 *
 *   code                       meaning                          decoded value     base afterwards
 *   -32768  KFPOS_D16_ABSENT   no range                         0                 unchanged
 *   -32767  KFPOS_D16_ESCAPE   the value is in the escape list  the listed value  the listed value
 *   -32766 ... 32767           delta                            base[e] + code    that sum
 *
 * The BASE is one int32 [max_anchors][n_tags] matrix per handle, zero at first, changed by D16 rounds only. The handle
 * keeps a host mirror (kfpos_delta_slot::base, what the encoder reads and moves) and a device copy (what the decode
 * kernel reads and moves); they are equal by construction, round for round, in submission order.
 * The ESCAPE LIST is (flat index, value) int32 pairs, strictly ascending by index.
 *
 * The decoded matrix is `v > 0 ? v : 0` of the values that were put, element for element: the canonical form of a range
 * matrix (the step kernels test `mm > 0` and nothing else), so a D16 round computes, bit for bit, what the plain round
 * with the caller's matrix computes.
 */
#ifndef KFPOS_D16_H
#define KFPOS_D16_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KFPOS_D16_ABSENT    (-32768)
#define KFPOS_D16_ESCAPE    (-32767)
#define KFPOS_D16_DELTA_MIN (-32766)
#define KFPOS_D16_DELTA_MAX 32767

/* what kfpos_slot_delta hands out: one slot opened for a D16 round */
typedef struct kfpos_delta_slot {
    int16_t *code;        /* pinned, [max_anchors][n_tags] */
    int32_t *esc;         /* pinned, [esc_capacity][2]: flat index, value */
    int32_t *n_esc;       /* entries used; kfpos_slot_delta sets it to 0 */
    int32_t  esc_capacity;/* max_anchors * n_tags: any matrix is representable */
    int32_t *base;        /* host mirror [max_anchors][n_tags], shared by the slots */
    int32_t  n_tags, max_anchors;
} kfpos_delta_slot;

/* Encode element e of the round: the only encoder rule there is.
 *   v <= 0                                   -> ABSENT
 *   d = (int64) v - base[e] in [-32766, 32767] -> the code is d
 *   otherwise                                -> ESCAPE, (e, v) appended to the escape list
 *   every present value: base[e] = v
 * Returns 0, or -1 when the escape list is full (nothing is written then).
 * CONTRACT: an element is put at most once per round (a second put would move the base twice), and the elements that
 * escape are put in ascending order of e -- or the producer sorts the list before it submits. */
static inline int kfpos_d16_put(const kfpos_delta_slot *d, int64_t e, int32_t v) {
    int64_t delta;
    if (v <= 0) {
        d->code[e] = (int16_t)KFPOS_D16_ABSENT;
        return 0;
    }
    delta = (int64_t)v - (int64_t)d->base[e];
    if (delta >= KFPOS_D16_DELTA_MIN && delta <= KFPOS_D16_DELTA_MAX) {
        d->code[e] = (int16_t)delta;
    } else {
        const int32_t k = *d->n_esc;
        if (k < 0 || k >= d->esc_capacity) return -1;
        d->esc[2 * (int64_t)k] = (int32_t)e;
        d->esc[2 * (int64_t)k + 1] = v;
        *d->n_esc = k + 1;
        d->code[e] = (int16_t)KFPOS_D16_ESCAPE;
    }
    d->base[e] = v;
    return 0;
}

/* The decoder in plain C: the text the kernel (k_decode_d16) is judged against. `esc` has passed the submit's checks
 * (indices ascending and inside the matrix, each pointing at an ESCAPE code unless its tag is skipped).
 *   dt   [n_tags] or NULL. With a dt array (KFPOS_SLOT_DT_PER_TAG) the codes and escape entries of a tag whose
 *        dt < 0 are not read: the tag decodes to 0 and its base is kept.
 *   base [max_anchors][n_tags], read and moved
 *   out  [max_anchors][n_tags]. An ESCAPE-coded element is written by its escape entry alone: one without an entry
 *        keeps what `out` held (the encoder never produces one). */
static inline void kfpos_d16_decode_ref(const int16_t *code, const int32_t *esc, int32_t n_esc, const double *dt,
                                        int32_t n_tags, int32_t max_anchors, int32_t *base, int32_t *out) {
    const int64_t n = (int64_t)n_tags * max_anchors;
    int64_t e;
    int32_t k;
    for (e = 0; e < n; ++e) {
        const int32_t c = code[e];
        if (dt && dt[e % n_tags] < 0.0) out[e] = 0;
        else if (c == KFPOS_D16_ABSENT) out[e] = 0;
        else if (c != KFPOS_D16_ESCAPE) out[e] = base[e] = (int32_t)((uint32_t)base[e] + (uint32_t)c);
    }
    for (k = 0; k < n_esc; ++k) {
        const int64_t i = esc[2 * (int64_t)k];
        if (dt && dt[i % n_tags] < 0.0) continue;
        out[i] = base[i] = esc[2 * (int64_t)k + 1];
    }
}

#ifdef __cplusplus
}
#endif
#endif /* KFPOS_D16_H */
