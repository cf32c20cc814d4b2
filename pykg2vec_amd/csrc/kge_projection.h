// kge_projection.h -- what the 1-N ("projection") models with their own descriptor share (kge_tucker.hip, kge_proje.hip, kge_conve.hip; DESIGN.md
// section 17): the dropout draw, the wave sum of their row kernels, the small host checks and the rank pass of kge_projection.hip.
//
// Dropout masks are never stored: forward and backward recompute them from Philox4x32-10 (kge_sampler_device.h).
//     key     = (low 32 bits of seed, high 32 bits of seed)
//     counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff),   word = row & 3
//     row     = position in the call's row list;   elem and site: the model's own (said at the top of its file)
// An element is KEPT iff its 32-bit word >= thr = floor(p * 2^32) (p the float dropout rate), and is then scaled by 1 / (1 - p) in fp32.
// Four consecutive rows share one Philox call.  With train = 0 or p = 0 nothing is drawn.
#pragma once
#include "kge_internal.h"
#include "kge_sampler_device.h"

namespace kge {

struct DropKey {
    uint32_t k0, k1, hi, lo;       // key, and the two offset words of the counter
};

__device__ __forceinline__ Philox drop_draw(const DropKey& k, uint32_t site, uint32_t elem, uint32_t rowgrp) {
    return philox4x32_10(elem, rowgrp, site | (k.hi << 2), k.lo, k.k0, k.k1);
}
__device__ __forceinline__ uint32_t drop_word(const Philox& x, int w) {   // selects: a dynamic index would put the words in memory
    return w == 0 ? x.c[0] : w == 1 ? x.c[1] : w == 2 ? x.c[2] : x.c[3];
}
// factor of element `elem` of row `row` at a row-wise site: 0 or scale
__device__ __forceinline__ float drop_row_factor(const DropKey& k, int site, int elem, int64_t row, uint32_t thr, float scale) {
    const Philox x = drop_draw(k, (uint32_t)site, (uint32_t)elem, (uint32_t)(row >> 2));
    return drop_word(x, (int)(row & 3)) >= thr ? scale : 0.0f;
}
// (not wave_sum of kge_device.h: that one is gsum<64>, whose order of additions differs -- swapping it in would change result bits)
__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

inline DropKey drop_key(uint64_t seed, uint64_t offset) {
    return DropKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(offset >> 32), (uint32_t)offset};
}
inline uint32_t drop_thr(float p) { return (uint32_t)((double)p * 4294967296.0); }
inline float drop_scale(float p) { return 1.0f / (1.0f - p); }
// the `n` rates of a descriptor and its Philox offset (the two high bits of the counter word carry the site)
inline int drop_check(const char* who, const float* p, int n, uint64_t offset) {
    for (int s = 0; s < n; ++s)
        if (!(p[s] >= 0.0f && p[s] < 1.0f)) {
            if (n == 1) set_error("%s: the dropout rate must be in [0, 1) (got %g)", who, (double)p[s]);
            else set_error("%s: dropout rate %d must be in [0, 1) (got %g)", who, s, (double)p[s]);
            return -1;
        }
    if (offset >> 62) { set_error("%s: the Philox offset must be below 2^62", who); return -1; }
    return 0;
}

// kge_projection.hip
int ws_check(const char* who, const void* ws, size_t have, size_t need);
int check_er_ids(const char* who, int64_t tot_entity, int64_t tot_relation, const int64_t* e, const int64_t* r, int64_t n, hipStream_t s);

// The filtered rank of a 1-N model: x = body(h, r) and body(t, r) WITHOUT dropout, then the head's rank per side (kge_head_1n_rank)
// in the [4, n] layout of kge_eval_ranks.  The model says its sizes and its body; `body` computes x [2n, dim] for the 2n rows
// e = [h; t], r = [rel; rel] of n triples in a workspace of body_bytes.
typedef int ProjectionBodyFn(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void* ws, size_t ws_bytes,
                             hipStream_t s);
struct ProjectionEval {
    int dim;
    int64_t tot_entity, tot_relation;
    const float* ent;
    size_t body_bytes;             // what `body` needs for the 2n rows of the call
    ProjectionBodyFn* body;
    const float* bias = nullptr;   // the head's bias [tot_entity] (ConvE's b); NULL = none (TuckER, ProjE_pointwise)
};
size_t projection_eval_workspace_bytes(const ProjectionEval& m, int64_t n);
int projection_eval_ranks(const char* who, const ProjectionEval& m, const void* desc, const int64_t* triples, int64_t n,
                          const int64_t* tail_off, const int32_t* tail_ids, const int64_t* head_off, const int32_t* head_ids, void* workspace,
                          size_t workspace_bytes, int32_t* ranks, int32_t* ties, void* stream);

}  // namespace kge
