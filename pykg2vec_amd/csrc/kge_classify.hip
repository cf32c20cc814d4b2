// kge_classify.hip -- triple classification (Socher et al. 2013): is (h, r, t) true, given the model's score and a per-relation
// threshold fitted on labelled validation triples?  Two entry points (include/kge_hip.h): kge_classification_fit chooses the
// thresholds and counts what the AUC needs, kge_classification_apply classifies and counts the confusion matrix.  Keys and
// thresholds: kge_classify_device.h.  Integer work only -- no float arithmetic, no float atomics -- so both are exact functions of
// the score bits and bit-identical from run to run.
//
// The fit, for n labelled scores over R relations:
//   k_cls_keys    one 64-bit key per triple: rel << 33 | score key << 1 | (1 - label), padded to a power of two with ~0; a relation
//                 id outside [0, R) becomes padding (the triple is ignored)
//   sort          the batched bitonic sort of kge_index.hip, one array: relations become segments, scores ascend in key order inside
//                 a segment, and the positives of a tie group (equal score keys) come before its negatives
//   scan          ONE segmented scan over the sorted POSITIONS carries, for position i: where its segment starts, the positives of its
//                 segment up to i (seg_pos), and the positives of its tie group up to i (grp_pos).  The operator is associative (the
//                 later operand's segment / group start resets the count), so the scan runs in the multi-launch form -- k_cls_block
//                 (aggregate of every 1024 positions), k_cls_sums (one workgroup scans the aggregates), k_cls_reduce (recompute the
//                 in-block scan, add the block's prefix).  No kernel waits on another workgroup.
//   k_cls_reduce  per position: a cut after i is valid when i ends its tie group and its score is a number; its value is
//                 2 * seg_pos - (i - seg_start + 1) = correct(i) - negatives(r), so the arg-max over cuts needs no second pass.  The
//                 choice per relation is an integer atomicMax on (value + 2^31) << 32 | ~(i + 1): the largest value, and among equal
//                 values the EARLIEST cut (the strictest threshold); the cut before everything (value 0, thr = -1) is the initial word
//                 and so the earliest of all.  A negative at i adds seg_pos - grp_pos to its relation's AUC wins (positives in
//                 strictly earlier tie groups) and grp_pos to its ties (positives sort first inside a group, so the group's positives
//                 all precede it).  The lanes of a wave that share a relation are combined with shuffles first: sorted positions
//                 make that nearly every lane, so a relation costs one atomic per wave whatever its share of the triples is -- the
//                 work is split by position, not by relation, and a relation holding a third of the triples serialises nothing.
//   k_cls_final   per relation: the threshold = the score key at the chosen position, and the fit row.
#include "kge_internal.h"
#include "kge_classify_device.h"

namespace kge {

namespace {

typedef unsigned long long u64;
constexpr int kClsBlock = 1024;
constexpr int64_t kClsMaxN = 1ll << 30;        // the sort's array length is an int
constexpr int64_t kClsMaxR = 1ll << 20;        // rel << 33 stays below the padding key
constexpr u64 kClsInitBest = ((u64)0x80000000u << 32) | 0xFFFFFFFFull;   // value 0 at the cut before everything

struct ClsState { int seg_start, seg_pos, grp_flag, grp_pos; };

__device__ __forceinline__ ClsState cls_identity() { return ClsState{-1, 0, 0, 0}; }
// `a` covers the positions in front of `b`
__device__ __forceinline__ ClsState cls_combine(const ClsState& a, const ClsState& b) {
    ClsState o;
    o.seg_start = a.seg_start > b.seg_start ? a.seg_start : b.seg_start;
    o.seg_pos = b.seg_start >= 0 ? b.seg_pos : a.seg_pos + b.seg_pos;
    o.grp_flag = a.grp_flag | b.grp_flag;
    o.grp_pos = b.grp_flag ? b.grp_pos : a.grp_pos + b.grp_pos;
    return o;
}

__device__ __forceinline__ ClsState cls_element(const u64* __restrict__ keys, int64_t i, int64_t n) {
    if (i >= n) return cls_identity();
    const u64 k = keys[i], prev = i ? keys[i - 1] : 0ull;
    const bool seg = i == 0 || (k >> 33) != (prev >> 33);
    const bool grp = i == 0 || (k >> 1) != (prev >> 1);
    const int pos = (int)(~k & 1ull);
    return ClsState{seg ? (int)i : -1, pos, grp ? 1 : 0, pos};
}

// inclusive scan of v over the 1024 threads of the block; *total = the block's aggregate (the same value in every thread)
__device__ __forceinline__ ClsState cls_block_scan(ClsState v, ClsState* total) {
    __shared__ ClsState s_wave[kClsBlock / 64];
    __shared__ ClsState s_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ClsState x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        ClsState y;
        y.seg_start = __shfl_up(x.seg_start, o, 64);
        y.seg_pos = __shfl_up(x.seg_pos, o, 64);
        y.grp_flag = __shfl_up(x.grp_flag, o, 64);
        y.grp_pos = __shfl_up(x.grp_pos, o, 64);
        if (lane >= o) x = cls_combine(y, x);
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        ClsState acc = cls_identity();
        for (int w = 0; w < kClsBlock / 64; ++w) { const ClsState t = s_wave[w]; s_wave[w] = acc; acc = cls_combine(acc, t); }
        s_total = acc;
    }
    __syncthreads();
    const ClsState out = cls_combine(s_wave[wave], x);
    *total = s_total;
    __syncthreads();   // s_wave / s_total may be rewritten by the next call
    return out;
}

__global__ __launch_bounds__(256) void k_cls_keys(const float* __restrict__ scores, const int64_t* __restrict__ rel,
                                                  const uint8_t* __restrict__ label, int64_t n, int64_t R, int higher, int P,
                                                  u64* __restrict__ keys) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    u64 key = ~0ull;
    if (j < n) {
        const int64_t r = rel[j];
        if (r >= 0 && r < R)
            key = ((u64)r << 33) | ((u64)cls_key(__float_as_uint(scores[j]), higher) << 1) | (label[j] ? 0ull : 1ull);
    }
    keys[j] = key;
}

// acc [R, 5] = {best word, positives, negatives, wins, ties}
__global__ __launch_bounds__(256) void k_cls_init(u64* __restrict__ acc, int64_t R) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= 5 * R) return;
    acc[j] = (j % 5 == 0) ? kClsInitBest : 0ull;
}

__global__ __launch_bounds__(kClsBlock) void k_cls_block(const u64* __restrict__ keys, int64_t n, ClsState* __restrict__ agg) {
    const int64_t i = (int64_t)blockIdx.x * kClsBlock + threadIdx.x;
    ClsState total;
    cls_block_scan(cls_element(keys, i, n), &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// exclusive scan of the block aggregates, one workgroup: pre[b] = everything in front of block b
__global__ __launch_bounds__(kClsBlock) void k_cls_sums(const ClsState* __restrict__ agg, int64_t n_blocks, ClsState* __restrict__ pre) {
    __shared__ ClsState s_carry;
    __shared__ ClsState s_last[kClsBlock / 64];
    if (threadIdx.x == 0) s_carry = cls_identity();
    __syncthreads();
    for (int64_t base = 0; base < n_blocks; base += kClsBlock) {
        const int64_t b = base + threadIdx.x;
        const ClsState v = b < n_blocks ? agg[b] : cls_identity();
        ClsState total;
        const ClsState incl = cls_block_scan(v, &total);
        const ClsState carry = s_carry;
        // exclusive = carry + (inclusive of the thread in front); thread 0 of the chunk takes the carry alone
        ClsState left;
        left.seg_start = __shfl_up(incl.seg_start, 1, 64);
        left.seg_pos = __shfl_up(incl.seg_pos, 1, 64);
        left.grp_flag = __shfl_up(incl.grp_flag, 1, 64);
        left.grp_pos = __shfl_up(incl.grp_pos, 1, 64);
        if ((threadIdx.x & 63) == 63) s_last[threadIdx.x >> 6] = incl;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) left = threadIdx.x ? s_last[(threadIdx.x >> 6) - 1] : cls_identity();
        if (b < n_blocks) pre[b] = cls_combine(carry, left);
        __syncthreads();
        if (threadIdx.x == 0) s_carry = cls_combine(carry, total);
        __syncthreads();
    }
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const u64 y = __shfl_xor(v, o, 64); v = y > v ? y : v; }
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kClsBlock) void k_cls_reduce(const u64* __restrict__ keys, int64_t n, int64_t R,
                                                          const ClsState* __restrict__ pre, u64* __restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * kClsBlock + threadIdx.x;
    ClsState total;
    const ClsState local = cls_block_scan(cls_element(keys, i, n), &total);
    const ClsState st = cls_combine(pre[blockIdx.x], local);
    const bool in = i < n;
    const u64 k = in ? keys[i] : ~0ull;
    const u64 r = k >> 33;
    const bool ok = in && r < (u64)R;
    const uint32_t sk = (uint32_t)(k >> 1);
    const bool positive = (k & 1ull) == 0ull;
    bool cut = ok && sk != kClsNanKey;
    if (cut && i + 1 < n) cut = (keys[i + 1] >> 1) != (k >> 1);
    u64 word = 0ull;   // below every real word: the initial one has value field 2^31
    if (cut) {
        const int value = 2 * st.seg_pos - ((int)i - st.seg_start + 1);
        word = ((u64)((uint32_t)value + 0x80000000u) << 32) | (u64)(uint32_t)~((uint32_t)i + 1u);
    }
    const u64 c_pos = ok && positive ? 1ull : 0ull, c_neg = ok && !positive ? 1ull : 0ull;
    const u64 wins = c_neg ? (u64)(st.seg_pos - st.grp_pos) : 0ull, ties = c_neg ? (u64)st.grp_pos : 0ull;
    // one atomic per (wave, relation): the loop runs once per distinct relation among the wave's 64 sorted positions
    const int lane = threadIdx.x & 63;
    const int rv = ok ? (int)r : -1;
    u64 pending = __ballot(ok);
    while (pending) {
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int r0 = __shfl(rv, leader, 64);
        const bool mine = rv == r0;
        const u64 w = wave_max(mine ? word : 0ull);
        const u64 p = wave_sum(mine ? c_pos : 0ull), q = wave_sum(mine ? c_neg : 0ull);
        const u64 a = wave_sum(mine ? wins : 0ull), b = wave_sum(mine ? ties : 0ull);
        if (lane == leader) {
            u64* row = acc + (int64_t)r0 * 5;
            if (w) atomicMax(row, w);
            if (p) atomicAdd(row + 1, p);
            if (q) atomicAdd(row + 2, q);
            if (a) atomicAdd(row + 3, a);
            if (b) atomicAdd(row + 4, b);
        }
        pending &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(256) void k_cls_final(const u64* __restrict__ keys, const u64* __restrict__ acc, int64_t R,
                                                   int64_t* __restrict__ thr, int64_t* __restrict__ fit) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const u64* row = acc + r * 5;
    const u64 best = row[0];
    const uint32_t ip1 = ~(uint32_t)best;   // chosen position + 1; 0 = the cut before everything
    const int64_t value = (int64_t)(uint32_t)(best >> 32) - 0x80000000ll;
    thr[r] = ip1 ? (int64_t)(uint32_t)(keys[ip1 - 1] >> 1) : -1;
    int64_t* f = fit + r * 6;
    f[0] = (int64_t)row[1]; f[1] = (int64_t)row[2]; f[2] = value + (int64_t)row[2];
    f[3] = (int64_t)row[3]; f[4] = (int64_t)row[4]; f[5] = 0;
}

// classify, and count the confusion matrix when labels are given: conf [R, 4] = {tp, fp, tn, fn}
__global__ __launch_bounds__(256) void k_cls_apply(const float* __restrict__ scores, const int64_t* __restrict__ rel,
                                                   const uint8_t* __restrict__ label, int64_t n, int64_t R,
                                                   const int64_t* __restrict__ thr, const uint8_t* __restrict__ seen,
                                                   int64_t thr_global, int higher, uint8_t* __restrict__ pred, u64* __restrict__ conf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int64_t r = in ? rel[i] : -1;
    const bool ok = in && r >= 0 && r < R;
    bool p = false;
    if (ok) p = cls_positive(cls_key(__float_as_uint(scores[i]), higher), seen[r] ? thr[r] : thr_global);
    if (in) pred[i] = p ? 1 : 0;
    if (!label) return;   // uniform over the grid
    int cell = -1;        // r * 4 + {tp, fp, tn, fn}
    if (ok) cell = (int)r * 4 + (label[i] ? (p ? 0 : 3) : (p ? 1 : 2));
    // the lanes of a wave that count into the same cell share one atomic
    const int lane = threadIdx.x & 63;
    u64 pending = __ballot(ok);
    while (pending) {
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int c0 = __shfl(cell, leader, 64);
        const u64 mine = __ballot(cell == c0);
        if (lane == leader) atomicAdd(conf + c0, (u64)__popcll(mine));
        pending &= ~mine;
    }
}

int cls_sort_length(int64_t n) { int P = 256; while (P < n) P <<= 1; return P; }

struct ClsPlan { u64* keys; ClsState* agg; ClsState* pre; u64* acc; size_t bytes; int P; int64_t n_blocks; };
ClsPlan cls_plan(void* ws, int64_t n, int64_t R) {
    ClsPlan p;
    p.P = cls_sort_length(n);
    p.n_blocks = n > 0 ? (n + kClsBlock - 1) / kClsBlock : 1;
    char* w = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    char* const w0 = w;
    p.keys = (u64*)w; w += align256((size_t)p.P * sizeof(u64));
    p.agg = (ClsState*)w; w += align256((size_t)p.n_blocks * sizeof(ClsState));
    p.pre = (ClsState*)w; w += align256((size_t)p.n_blocks * sizeof(ClsState));
    p.acc = (u64*)w; w += align256((size_t)R * 5 * sizeof(u64));
    p.bytes = (size_t)(w - w0) + 256;
    return p;
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

int64_t kge_classification_sort_length(int64_t n) {
    if (n < 0 || n > kClsMaxN) return 0;
    return cls_sort_length(n);
}

size_t kge_classification_fit_workspace_bytes(int64_t n, int64_t R) {
    if (n < 0 || n > kClsMaxN || R < 1 || R >= kClsMaxR) return 0;
    return cls_plan(nullptr, n, R).bytes;
}

int kge_classification_fit(const float* scores, const int64_t* rel, const uint8_t* label, int64_t n, int64_t R, int32_t higher_is_better,
                           void* workspace, size_t workspace_bytes, int64_t* thr, int64_t* fit, void* stream) {
    const char* who = "kge_classification_fit";
    if (n < 0) { set_error("%s: n = %lld is negative", who, (long long)n); return -1; }
    if (n > kClsMaxN) { set_error("%s: n = %lld exceeds 2^30, the sort's array length is an int", who, (long long)n); return -1; }
    if (R < 1 || R >= kClsMaxR) { set_error("%s: R = %lld outside 1..2^20-1 (the sort key holds rel << 33)", who, (long long)R); return -1; }
    if (n > 0 && (!scores || !rel || !label)) { set_error("%s: null %s", who, !scores ? "scores" : !rel ? "rel" : "label"); return -1; }
    if (!thr || !fit) { set_error("%s: null %s", who, !thr ? "thr" : "fit"); return -1; }
    if (!workspace) { set_error("%s: null workspace", who); return -1; }
    const ClsPlan p = cls_plan(workspace, n, R);
    if (workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_classification_fit_workspace_bytes = %zu)", who, workspace_bytes, p.bytes);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) if (int rc = debug_check_ids(who, "rel", rel, n, 1, 0, R, s)) return rc;
    hipLaunchKernelGGL(k_cls_init, dim3((unsigned)((5 * R + 255) / 256)), dim3(256), 0, s, p.acc, R);
    int rc = check_launch("k_cls_init");
    if (rc) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(k_cls_keys, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0, s, scores, rel, label, n, R,
                           higher_is_better ? 1 : 0, p.P, p.keys);
        if ((rc = check_launch("k_cls_keys"))) return rc;
        if ((rc = sort_batched(p.keys, 1, p.P, s))) return rc;
        hipLaunchKernelGGL(k_cls_block, dim3((unsigned)p.n_blocks), dim3(kClsBlock), 0, s, p.keys, n, p.agg);
        hipLaunchKernelGGL(k_cls_sums, dim3(1), dim3(kClsBlock), 0, s, p.agg, p.n_blocks, p.pre);
        hipLaunchKernelGGL(k_cls_reduce, dim3((unsigned)p.n_blocks), dim3(kClsBlock), 0, s, p.keys, n, R, p.pre, p.acc);
        if ((rc = check_launch("k_cls_reduce"))) return rc;
    }
    hipLaunchKernelGGL(k_cls_final, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, p.keys, p.acc, R, thr, fit);
    return check_launch("k_cls_final");
}

int kge_classification_apply(const float* scores, const int64_t* rel, const uint8_t* label, int64_t n, int64_t R, int32_t higher_is_better,
                             const int64_t* thr, const uint8_t* seen, int64_t thr_global, uint8_t* pred, int64_t* conf, void* stream) {
    const char* who = "kge_classification_apply";
    if (n < 0) { set_error("%s: n = %lld is negative", who, (long long)n); return -1; }
    if (R < 1 || R >= kClsMaxR) { set_error("%s: R = %lld outside 1..2^20-1", who, (long long)R); return -1; }
    if (n > 0 && (!scores || !rel || !pred)) { set_error("%s: null %s", who, !scores ? "scores" : !rel ? "rel" : "pred"); return -1; }
    if (!thr || !seen) { set_error("%s: null %s", who, !thr ? "thr" : "seen"); return -1; }
    if (label && !conf) { set_error("%s: labels without conf", who); return -1; }
    if (thr_global < -1 || thr_global > 0xFFFFFFFFll) { set_error("%s: thr_global = %lld is no key (-1..2^32-1)", who, (long long)thr_global); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) if (int rc = debug_check_ids(who, "rel", rel, n, 1, 0, R, s)) return rc;
    if (label) {
        hipError_t e = hipMemsetAsync(conf, 0, (size_t)R * 4 * sizeof(int64_t), s);
        if (e != hipSuccess) { set_error("%s: memset: %s", who, hipGetErrorString(e)); return -2; }
    }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_cls_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scores, rel, label, n, R, thr, seen, thr_global,
                       higher_is_better ? 1 : 0, pred, (u64*)conf);
    return check_launch("k_cls_apply");
}

}  // extern "C"
