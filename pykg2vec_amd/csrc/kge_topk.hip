// kge_topk.hip -- row select of the batched link prediction: the k most plausible live candidates of every score row, in ONE total
// order (better score first, lower candidate id first among equal scores), so the answer is an exact function of the inputs.
//
//   key      an order-preserving unsigned image of the score: the sign-flip transform (inverted for `largest`), -0.0 folded onto
//            +0.0 first.  Every number lands in [kFirst, kLast]; a live NaN takes kNan = MAX - 1 and a masked candidate
//            kMasked = MAX, both above every number in both directions.
//   mask     workspace bit mask [nq, ceil(n_cand / 32)], zeroed and then set by k_topk_mask with integer atomicOr (the result does
//            not depend on the order); ids outside [0, n_cand) and the row's keep id set nothing.
//   select   one 256-thread workgroup per row.  A byte-wise radix select over the key (histogram in LDS with integer atomics, whose
//            sums do not depend on the order) finds the key T of the kk-th candidate, kk = min(k, live), and how many of the keys
//            equal to T belong to the answer; T < kMasked because the masked keys are the row's n_cand - live largest.  One more
//            sweep in id order compacts (key, id) of every key below T and of the FIRST keys equal to T into LDS at its id-ordered
//            slot (wave ballots + one barrier per 256 candidates), a bitonic network sorts the at most 1024 pairs by (key, id),
//            and the scores are read back by id, so out_scores holds their bit patterns.
// Launches per call: one memset and k_topk_mask (masked calls only), then k_topk_select -- whatever nq is.  Elements in
// [n_cand, row_stride) are never read.  No float arithmetic and no float atomics anywhere.
#include "kge_internal.h"

namespace kge {

namespace {

constexpr int kTopkBlock = 256;
constexpr int kTopkWaves = kTopkBlock / 64;

template <typename KeyT> struct TopkKey;
template <> struct TopkKey<uint32_t> {
    static constexpr uint32_t sign = 0x80000000u, inf = 0x7f800000u, max = 0xffffffffu, qnan = 0x7fc00000u;
};
template <> struct TopkKey<uint64_t> {
    static constexpr uint64_t sign = 0x8000000000000000ull, inf = 0x7ff0000000000000ull, max = 0xffffffffffffffffull,
                              qnan = 0x7ff8000000000000ull;
};

template <typename KeyT>
__device__ __forceinline__ KeyT topk_key(KeyT bits, int largest) {
    typedef TopkKey<KeyT> C;
    if ((bits & ~C::sign) > C::inf) return C::max - 1;            // NaN: after every number, before the masked
    if (bits == C::sign) bits = 0;                                // -0.0 == +0.0
    const KeyT asc = (bits & C::sign) ? ~bits : (bits | C::sign); // ascending in the score
    return largest ? ~asc : asc;                                  // numbers stay inside [~(inf | sign), inf | sign] either way
}

__device__ __forceinline__ bool topk_masked(const uint32_t* __restrict__ mrow, unsigned i) {
    return mrow && ((mrow[i >> 5] >> (i & 31)) & 1u);
}

}  // namespace

// one wave per row: the row's skip ids -> bits of its mask row
__global__ void __launch_bounds__(kTopkBlock) k_topk_mask(const int64_t* __restrict__ skip_off, const int32_t* __restrict__ skip_ids,
                                                            const int64_t* __restrict__ keep, int64_t nq, int64_t n_cand, int64_t W,
                                                            uint32_t* __restrict__ mask) {
    const int64_t q = (int64_t)blockIdx.x * kTopkWaves + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int64_t lo = skip_off[q], hi = skip_off[q + 1];
    const int64_t kept = keep ? keep[q] : -1;
    uint32_t* mrow = mask + q * W;
    for (int64_t j = lo + (threadIdx.x & 63); j < hi; j += 64) {
        const int64_t id = skip_ids[j];
        if (id >= 0 && id < n_cand && id != kept) atomicOr(mrow + (id >> 5), 1u << (id & 31));
    }
}

template <typename KeyT>
__global__ void __launch_bounds__(kTopkBlock) k_topk_select(const KeyT* __restrict__ scores, int64_t n_cand64, int64_t row_stride, int k,
                                                              int largest, const uint32_t* __restrict__ mask, int64_t W,
                                                              int32_t* __restrict__ out_ids, KeyT* __restrict__ out_scores,
                                                              int32_t* __restrict__ out_count) {
    typedef TopkKey<KeyT> C;
    __shared__ KeyT s_key[KGE_TOPK_MAX];
    __shared__ int32_t s_id[KGE_TOPK_MAX];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[2][kTopkWaves][2];
    __shared__ uint32_t s_pick[2];
    __shared__ uint32_t s_dead;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const unsigned n_cand = (unsigned)n_cand64;
    const KeyT* __restrict__ row = scores + q * row_stride;
    const uint32_t* __restrict__ mrow = mask ? mask + q * W : nullptr;

    // ---- live candidates of the row
    if (tid == 0) s_dead = 0;
    s_hist[tid] = 0;
    __syncthreads();
    if (mrow) {
        uint32_t dead = 0;
        for (unsigned w = tid; w < (unsigned)W; w += kTopkBlock) dead += __popc(mrow[w]);
        if (dead) atomicAdd(&s_dead, dead);
    }
    __syncthreads();
    const unsigned live = n_cand - s_dead;
    const unsigned kk = live < (unsigned)k ? live : (unsigned)k;

    if (kk > 0) {
        // ---- radix select: T = key of the candidate of 0-based place kk - 1 in key order, most significant byte first
        KeyT prefix = 0;
        uint32_t rem = kk - 1;
        for (int shift = (int)sizeof(KeyT) * 8 - 8; shift >= 0; shift -= 8) {
            for (unsigned i = tid; i < n_cand; i += kTopkBlock) {
                const KeyT key = topk_masked(mrow, i) ? C::max : topk_key<KeyT>(row[i], largest);
                // (shift + 8 == key width on the first pass: every key takes part)
                const bool in = shift + 8 == (int)sizeof(KeyT) * 8 || (key >> (shift + 8)) == (prefix >> (shift + 8));
                if (in) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            // exclusive scan of the 256 bins, one per thread
            const uint32_t c = s_hist[tid];
            uint32_t inc = c;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(inc, d);
                if (lane >= d) inc += up;
            }
            if (lane == 63) s_wave[0][wave][0] = inc;
            __syncthreads();
            uint32_t base = 0;
            for (int w = 0; w < wave; ++w) base += s_wave[0][w][0];
            const uint32_t excl = base + inc - c;
            if (rem >= excl && rem < excl + c) { s_pick[0] = (uint32_t)tid; s_pick[1] = rem - excl; }   // exactly one bin holds place rem
            s_hist[tid] = 0;
            __syncthreads();
            prefix |= (KeyT)s_pick[0] << shift;
            rem = s_pick[1];
        }
        const KeyT T = prefix;
        const uint32_t need = rem + 1;          // of the keys equal to T, the first `need` by id belong to the answer
        // (kk - need keys lie strictly below T)

        // ---- sentinels behind the answer, up to the bitonic network's power of two
        unsigned P = 1;
        while (P < kk) P <<= 1;
        for (unsigned j = kk + tid; j < P; j += kTopkBlock) { s_key[j] = C::max; s_id[j] = 0x7fffffff; }

        // ---- compaction in id order: a key below T sits at #(below before it) + min(#(equal before it), need)
        uint32_t run_less = 0, run_eq = 0;
        int par = 0;
        for (unsigned i0 = 0; i0 < n_cand; i0 += kTopkBlock, par ^= 1) {
            const unsigned i = i0 + tid;
            KeyT key = C::max;
            if (i < n_cand && !topk_masked(mrow, i)) key = topk_key<KeyT>(row[i], largest);
            const bool less = key < T, eq = key == T;      // T < C::max: neither holds for the masked and the out-of-range
            const unsigned long long bl = __ballot(less), be = __ballot(eq);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (lane == 0) { s_wave[par][wave][0] = (uint32_t)__popcll(bl); s_wave[par][wave][1] = (uint32_t)__popcll(be); }
            __syncthreads();
            uint32_t less_before = run_less + (uint32_t)__popcll(bl & below), eq_before = run_eq + (uint32_t)__popcll(be & below);
#pragma unroll
            for (int w = 0; w < kTopkWaves; ++w) {
                const uint32_t l = s_wave[par][w][0], e = s_wave[par][w][1];
                if (w < wave) { less_before += l; eq_before += e; }
                run_less += l;
                run_eq += e;
            }
            if (less || (eq && eq_before < need)) {
                const uint32_t pos = less_before + (eq_before < need ? eq_before : need);
                s_key[pos] = key;
                s_id[pos] = (int32_t)i;
            }
        }
        __syncthreads();

        // ---- bitonic sort of the P pairs by (key, id)
        for (unsigned size = 2; size <= P; size <<= 1) {
            for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
                for (unsigned t = tid; t < (P >> 1); t += kTopkBlock) {
                    const unsigned a = 2 * t - (t & (stride - 1)), b = a + stride;
                    const KeyT ka = s_key[a], kb = s_key[b];
                    const int32_t ia = s_id[a], ib = s_id[b];
                    const bool a_after_b = ka > kb || (ka == kb && ia > ib);
                    const bool ascending = (a & size) == 0;
                    if (a_after_b == ascending) { s_key[a] = kb; s_key[b] = ka; s_id[a] = ib; s_id[b] = ia; }
                }
                __syncthreads();
            }
        }
    }

    // ---- the row's answer: ids, the scores' bit patterns, padding
    for (unsigned j = tid; j < (unsigned)k; j += kTopkBlock) {
        int32_t id = -1;
        KeyT bits = C::qnan;
        if (j < kk) { id = s_id[j]; bits = row[id]; }
        out_ids[q * k + j] = id;
        out_scores[q * k + j] = bits;
    }
    if (tid == 0) out_count[q] = (int32_t)kk;
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_topk_workspace_bytes(int64_t nq, int64_t n_cand, int masked) {
    if (!masked || nq <= 0 || n_cand <= 0) return 0;
    return align256((size_t)nq * (size_t)((n_cand + 31) / 32) * sizeof(uint32_t)) + 256;   // + 256: the caller's pointer is aligned up
}

int kge_topk_rows(const void* scores, int dtype, int64_t nq, int64_t n_cand, int64_t row_stride, int32_t k, int largest,
                  const int64_t* skip_off, const int32_t* skip_ids, const int64_t* keep, void* workspace, size_t workspace_bytes,
                  int32_t* out_ids, void* out_scores, int32_t* out_count, void* stream) {
    const char* who = "kge_topk_rows";
    if (k < 1 || k > KGE_TOPK_MAX) { set_error("%s: k = %d outside 1..%d (KGE_TOPK_MAX)", who, (int)k, KGE_TOPK_MAX); return -1; }
    if (dtype != 0 && dtype != 1) { set_error("%s: dtype = %d (0 = float32, 1 = float64)", who, dtype); return -1; }
    if (nq < 0 || nq > 0x7fffffffll) { set_error("%s: nq = %lld outside 0..2^31-1", who, (long long)nq); return -1; }
    if (n_cand < 1 || n_cand > 0x7fffff00ll) { set_error("%s: n_cand = %lld outside 1..2^31-257 (candidate ids are int32)", who, (long long)n_cand); return -1; }
    if (row_stride < n_cand) { set_error("%s: row_stride = %lld < n_cand = %lld", who, (long long)row_stride, (long long)n_cand); return -1; }
    if (skip_off && !skip_ids) { set_error("%s: skip_off without skip_ids", who); return -1; }
    const bool masked = skip_off != nullptr;
    if (masked && (!workspace || workspace_bytes < kge_topk_workspace_bytes(nq, n_cand, 1))) {
        set_error("%s: workspace too small (%zu bytes, kge_topk_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0,
                  kge_topk_workspace_bytes(nq, n_cand, 1));
        return -1;
    }
    if (nq == 0) return 0;
    if (!scores || !out_ids || !out_scores || !out_count) { set_error("%s: null scores / out_ids / out_scores / out_count", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t W = (n_cand + 31) / 32;
    uint32_t* mask = nullptr;
    if (masked) {
        mask = (uint32_t*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
        hipError_t e = hipMemsetAsync(mask, 0, (size_t)nq * (size_t)W * sizeof(uint32_t), s);
        if (e != hipSuccess) { set_error("%s: memset: %s", who, hipGetErrorString(e)); return -2; }
        hipLaunchKernelGGL(k_topk_mask, dim3((unsigned)((nq + kTopkWaves - 1) / kTopkWaves)), dim3(kTopkBlock), 0, s, skip_off, skip_ids, keep,
                           nq, n_cand, W, mask);
        if (int rc = check_launch("k_topk_mask")) return rc;
    }
    if (dtype == 0)
        hipLaunchKernelGGL((k_topk_select<uint32_t>), dim3((unsigned)nq), dim3(kTopkBlock), 0, s, (const uint32_t*)scores, n_cand, row_stride,
                           (int)k, largest ? 1 : 0, mask, W, out_ids, (uint32_t*)out_scores, out_count);
    else
        hipLaunchKernelGGL((k_topk_select<uint64_t>), dim3((unsigned)nq), dim3(kTopkBlock), 0, s, (const uint64_t*)scores, n_cand, row_stride,
                           (int)k, largest ? 1 : 0, mask, W, out_ids, (uint64_t*)out_scores, out_count);
    return check_launch("k_topk_select");
}

}  // extern "C"
