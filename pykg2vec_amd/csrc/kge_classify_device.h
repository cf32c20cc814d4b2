// kge_classify_device.h -- score orientation and key space of triple classification, shared by the fit, the classify-and-count
// pass (kge_classify.hip) and nothing else: every decision of the protocol is a comparison of these keys.
//
// A score becomes a 32-bit unsigned key; a SMALLER key is MORE plausible.  The map is the sign-flip transform of the float32 bits
// (ascending in the score), complemented for a higher-is-better model, with -0.0 folded onto +0.0 first so that key equality is float
// equality.  Every NaN takes kClsNanKey = 0xFFFFFFFF: numbers land in [0x007FFFFF, 0xFF800000] in both orientations, so a NaN sorts
// after every number, never ties with one, and is never classified positive (cls_positive).  This is the convention of topk_key
// (kge_topk.hip) except for the NaN's key: there a live NaN is MAX - 1 because MAX is the masked candidate; here nothing is masked.
//
// A threshold is an int64 in the same space: -1 = nothing is positive, otherwise triple i is positive iff key_i <= thr.  A threshold
// is always the key of an observed score, never a midpoint, so fit and classification are exact functions of the score bits.
#pragma once
#include <stdint.h>

namespace kge {

constexpr uint32_t kClsNanKey = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint32_t cls_key(uint32_t bits, int higher_is_better) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return kClsNanKey;
    if (bits == 0x80000000u) bits = 0u;
    const uint32_t asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return higher_is_better ? ~asc : asc;
}

__host__ __device__ __forceinline__ bool cls_positive(uint32_t key, int64_t thr) {
    return key != kClsNanKey && (int64_t)key <= thr;   // thr = -1: false for every key
}

}  // namespace kge
