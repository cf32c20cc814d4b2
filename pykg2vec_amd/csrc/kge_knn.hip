// kge_knn.hip -- nearest neighbours in embedding space: the k nearest live table rows of every query row under dot, cosine or
// Euclidean distance, in the total order of kge_topk_rows (better score first, lower id first among equal scores, NaN last).  The
// select sits INSIDE the matrix-core sweep: no [nq, n_rows] score block is ever written.
//
//   k_knn_norms   |row|^2 (L2) or |row| (cosine) of every table and query row: one wave per row, lanes stride the row, xor butterfly --
//                 a fixed order.  Not launched for the dot metric.
//   k_knn_sweep   a workgroup owns a tile of 64 (k <= 32) or 32 queries and one slab of the candidate range (blockIdx.y of S).  Per
//                 step: 128 candidates x the query tile on mfma_f32_32x32x2f32 (exact f32: an fmaf chain over dim), operands through
//                 k-major LDS in slabs of 32, the tail of dim zero-filled.  The accumulator becomes the metric's score, the score the
//                 ascending unsigned key of the row select (NaN at MAX - 1), and the pair (key << 32 | id) is compared with the query's
//                 threshold: the k-th best pair of its buffer at the last compaction, MAX before.  Only p < thr is appended (an integer
//                 LDS add hands out the slot; which slot carries no meaning).  A lane that finds the buffer full keeps the candidate
//                 pending; full buffers are compacted (below) and the pending ones are tried again against the tighter threshold, until
//                 none is left.  Whatever is turned away is behind k pairs that were seen, so it is not in the answer: the result is
//                 the k best pairs of the slab however the appends interleave.
//   compaction    one wave per query, by rank: every lane counts the buffer's pairs below its own (pairs are distinct: ids are), pairs
//                 of rank < k go to place [rank] -- sorted, no power-of-two padding -- and the pair at [k - 1] is the new threshold.
//   k_knn_finish  one workgroup per query: bitonic sort of the S partial lists under the same order.  L2 recomputes the winners'
//                 distances as sqrt(sum (q_i - c_i)^2) (one wave per winner, fixed order) and sorts again by (returned bits, id), so
//                 identical rows are at exactly 0.0 and no returned distance carries the expansion's cancellation.
// Launches per call: k_knn_norms (cosine, L2), k_knn_sweep, k_knn_finish -- whatever nq and n_rows are.  The only atomics are integer
// LDS adds whose results are slot numbers.
#include <cstdio>
#include "kge_internal.h"

namespace kge {

namespace {

constexpr int kKnnBlock = 256;
constexpr int kKnnWaves = kKnnBlock / 64;
constexpr int kKnnCT = 128;              // candidates per step: 32 per wave
constexpr int kKnnKS = 32;               // dim slab of one LDS fill
constexpr int kKnnCS = kKnnCT + 4;       // k-major operand rows, padded
constexpr int kKnnExtra = 32;            // buffer places behind the k kept pairs
constexpr int kKnnFinishMax = 2048;      // pairs k_knn_finish sorts in LDS: S * k stays below
constexpr int kKnnTargetGroups = 512;    // the split fills the device from one query tile on: two workgroups per CU are resident
constexpr unsigned long long kKnnNone = ~0ull;

__device__ __forceinline__ uint32_t knn_key(float score, bool largest) {
    uint32_t bits = __float_as_uint(score);
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xfffffffeu;          // NaN: after every number
    if (bits == 0x80000000u) bits = 0;                                  // -0.0 == +0.0
    const uint32_t asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return largest ? ~asc : asc;
}

__device__ __forceinline__ float knn_unkey(uint32_t key, bool largest) {
    if (key == 0xfffffffeu) return __uint_as_float(0x7fc00000u);
    const uint32_t asc = largest ? ~key : key;
    return __uint_as_float((asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc);
}

__device__ __forceinline__ float knn_wave_sum(float s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

// Ranks of a wave's pairs among themselves: lane l holds pairs e[j] = buffer[l + 64 j] (MAX from place n on), r[j] becomes the number
// of the n pairs below e[j].  The pairs travel through lane reads of a uniform lane, not through LDS: a handful of instructions
// per pair.
template <int NG>   // 64 * NG buffer places at most
__device__ __forceinline__ void knn_ranks(const unsigned long long (&e)[NG], int n, int (&r)[NG]) {
#pragma unroll
    for (int j = 0; j < NG; ++j) r[j] = 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int m = n - 64 * g < 64 ? n - 64 * g : 64;
        const int lo = (int)(uint32_t)e[g], hi = (int)(uint32_t)(e[g] >> 32);
        for (int i = 0; i < m; ++i) {
            const unsigned long long v = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(hi, i) << 32) |
                                         (uint32_t)__builtin_amdgcn_readlane(lo, i);
#pragma unroll
            for (int j = 0; j < NG; ++j) r[j] += v < e[j] ? 1 : 0;
        }
    }
}

// the query tile's share of the dynamic LDS, in bytes: buffers, thresholds, operand slabs, counters, the tile's candidate norms
inline size_t knn_sweep_lds(int qt, int cap) {
    return (size_t)qt * cap * 8 + (size_t)qt * 8 + (size_t)kKnnKS * kKnnCS * 4 + (size_t)kKnnKS * (qt + 4) * 4 + (size_t)qt * 4 +
           (size_t)kKnnCT * 4;
}

}  // namespace

__global__ void __launch_bounds__(kKnnBlock) k_knn_norms(const float* __restrict__ table, int64_t n_rows, int64_t table_stride,
                                                           const float* __restrict__ queries, int64_t nq, int64_t query_stride, int dim,
                                                           int root, float* __restrict__ tnorm, float* __restrict__ qnorm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kKnnWaves + (threadIdx.x >> 6);
    if (row >= n_rows + nq) return;
    const float* __restrict__ src = row < n_rows ? table + row * table_stride : queries + (row - n_rows) * query_stride;
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) { const float v = src[i]; s = fmaf(v, v, s); }
    s = knn_wave_sum(s);
    if (root) s = sqrtf(s);
    if (lane == 0) { if (row < n_rows) tnorm[row] = s; else qnorm[row - n_rows] = s; }
}

template <int NQ, int METRIC>   // query tile of 32 * NQ
__global__ void __launch_bounds__(kKnnBlock) k_knn_sweep(const float* __restrict__ table, int64_t n_rows, int dim, int64_t table_stride,
                                                           const float* __restrict__ queries, int64_t nq, int64_t query_stride,
                                                           const int64_t* __restrict__ self_ids, int k, int cap,
                                                           int tiles_per, int ctiles, const float* __restrict__ tnorm,
                                                           const float* __restrict__ qnorm, unsigned long long* __restrict__ part) {
    constexpr int QT = 32 * NQ, QS = QT + 4, NLQ = QT / 8, NG = NQ == 2 ? 1 : 3;   // (the 64-query tile keeps 64 places: knn_plan)
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    extern __shared__ unsigned long long knn_smem[];
    unsigned long long* s_buf = knn_smem;                         // [QT][cap]
    unsigned long long* s_thr = s_buf + (size_t)QT * cap;         // [QT]
    float* sC = reinterpret_cast<float*>(s_thr + QT);             // [KS][CS]
    float* sQ = sC + kKnnKS * kKnnCS;                             // [KS][QS]
    int* s_cnt = reinterpret_cast<int*>(sQ + kKnnKS * QS);        // [QT]
    float* s_cn = reinterpret_cast<float*>(s_cnt + QT);           // [CT]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, lk = lane >> 5;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int S = gridDim.y, sp = blockIdx.y;
    const int t0 = sp * tiles_per, t1 = (t0 + tiles_per < ctiles) ? t0 + tiles_per : ctiles;   // tiles of 128 ids: below 2^24
    const int nslab = (dim - 1) / kKnnKS + 1;
    constexpr bool largest = METRIC != KGE_KNN_L2;

    for (int i = tid; i < QT; i += kKnnBlock) { s_cnt[i] = 0; s_thr[i] = kKnnNone; }

    // the lane's query columns (candidate ids fit 31 bits; a query past nq keeps threshold 0: nothing is below it)
    float qn[NQ];
    int self[NQ];
    bool qok[NQ];
#pragma unroll
    for (int ni = 0; ni < NQ; ++ni) {
        const int64_t q = q0 + ni * 32 + li;
        qok[ni] = q < nq;
        qn[ni] = (qok[ni] && METRIC != KGE_KNN_DOT) ? qnorm[q] : 0.f;
        const int64_t own = (qok[ni] && self_ids) ? self_ids[q] : -1;
        self[ni] = (own >= 0 && own < n_rows) ? (int)own : -1;
    }
    const int n_cand = (int)n_rows;

    // global -> registers -> LDS, one step ahead of the matrix cores
    // The loads are unconditional, from addresses clamped into the row range and the row: a load under a condition is followed by a
    // select, and the select by a wait -- twelve memory round trips in a row per step instead of one.  Which elements are
    // zeros (past n_rows, nq or dim) is remembered in a bit mask and applied when the registers go to LDS.
    float rc[16], rq[NLQ];
    uint32_t ld_ok = 0;   // bit i: rc[i] is an element of the table, bit 16 + i: rq[i] of the queries
    int ld_t = t0, ld_s = 0;
    const int q_last = (int)((nq - 1 - q0 < QT - 1) ? nq - 1 - q0 : QT - 1);   // the tile's last query row (nq > q0: the grid covers nq)
    auto load_step = [&]() __attribute__((always_inline)) {
        const int kd = ld_s * kKnnKS + (tid & 31);
        const bool kin = kd < dim;
        const int kc = kin ? kd : dim - 1;
        ld_ok = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = ld_t * kKnnCT + (tid >> 5) + 8 * i;
            const bool in = c < n_cand;
            rc[i] = table[(int64_t)(in ? c : n_cand - 1) * table_stride + kc];
            ld_ok |= (kin && in) ? 1u << i : 0u;
        }
#pragma unroll
        for (int i = 0; i < NLQ; ++i) {
            const int ql = (tid >> 5) + 8 * i;
            const bool in = ql <= q_last;
            rq[i] = queries[(q0 + (in ? ql : q_last)) * query_stride + kc];
            ld_ok |= (kin && in) ? 65536u << i : 0u;
        }
        if (++ld_s == nslab) { ld_s = 0; ++ld_t; }
    };

    f32x16 acc[NQ];
#pragma unroll
    for (int ni = 0; ni < NQ; ++ni) acc[ni] = f32x16{0};
    if (t0 < t1) load_step();
    __syncthreads();
    for (int ct = t0; ct < t1; ++ct) {
        // the tile's candidate norms: asked for now, parked in LDS behind the slabs
        float cn_mine = 0.f;
        if (METRIC != KGE_KNN_DOT && tid < kKnnCT) { const int c = ct * kKnnCT + tid; cn_mine = tnorm[c < n_cand ? c : n_cand - 1]; }
        for (int sl = 0; sl < nslab; ++sl) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sC[(tid & 31) * kKnnCS + (tid >> 5) + 8 * i] = (ld_ok >> i) & 1u ? rc[i] : 0.f;
#pragma unroll
            for (int i = 0; i < NLQ; ++i) sQ[(tid & 31) * QS + (tid >> 5) + 8 * i] = (ld_ok >> (16 + i)) & 1u ? rq[i] : 0.f;
            __syncthreads();
            if (ld_t < t1) load_step();
#pragma unroll
            for (int kk = 0; kk < kKnnKS; kk += 2) {
                const float a = sC[(kk + lk) * kKnnCS + wave * 32 + li];
#pragma unroll
                for (int ni = 0; ni < NQ; ++ni)
                    acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sQ[(kk + lk) * QS + ni * 32 + li], acc[ni], 0, 0, 0);
            }
            __syncthreads();   // the slab is consumed: the next fill may overwrite it
        }
        if (METRIC != KGE_KNN_DOT) {
            if (tid < kKnnCT) s_cn[tid] = cn_mine;
            __syncthreads();
        }
        // ---- the tile's scores are complete: the lane owns query column (ni, li), its 16 registers are candidate rows
        const int cbase = ct * kKnnCT + wave * 32 + 4 * lk;
        uint32_t pend = NQ == 2 ? 0xffffffffu : 0xffffu;   // bit ni * 16 + reg: still to be offered to the query's buffer
        for (;;) {
            unsigned long long thr[NQ];
#pragma unroll
            for (int ni = 0; ni < NQ; ++ni) thr[ni] = qok[ni] ? s_thr[ni * 32 + li] : 0ull;
            uint32_t left = 0;
            // four registers at a time; the accumulators turn by four places per round (a whole turn in all), so that the body
            // names registers 0..3 only: a rolled loop, a quarter of the code and of the values in flight
#pragma unroll 1
            for (int r4 = 0; r4 < 4; ++r4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = cbase + j + 8 * r4;
                    const bool cok = c < n_cand;
                    const float cn = METRIC != KGE_KNN_DOT ? s_cn[wave * 32 + 4 * lk + j + 8 * r4] : 0.f;
#pragma unroll
                    for (int ni = 0; ni < NQ; ++ni) {
                        const uint32_t bit = 1u << (ni * 16 + 4 * r4 + j);
                        const float dot = acc[ni][j];
                        float sc = dot;
                        if constexpr (METRIC == KGE_KNN_COSINE) {
                            const float den = qn[ni] * cn;
                            sc = den == 0.f ? dot * 0.f : dot / den;     // a zero-norm row: cosine 0 (NaN stays NaN)
                        } else if constexpr (METRIC == KGE_KNN_L2) {
                            sc = (qn[ni] + cn) - 2.0f * dot;
                            sc = sc < 0.f ? 0.f : sc;                    // (a comparison, not fmaxf: NaN stays NaN)
                        }
                        const unsigned long long p = ((unsigned long long)knn_key(sc, largest) << 32) | (uint32_t)c;
                        if ((pend & bit) && cok && c != self[ni] && p < thr[ni]) {
                            const int slot = atomicAdd(&s_cnt[ni * 32 + li], 1);
                            if (slot < cap) s_buf[(ni * 32 + li) * cap + slot] = p;
                            else left |= bit;
                        }
                    }
                }
#pragma unroll
                for (int ni = 0; ni < NQ; ++ni)
                    acc[ni] = __builtin_shufflevector(acc[ni], acc[ni], 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3);
            }
            pend = left;
            const int any = __syncthreads_or(pend != 0);
            // compaction: with pending candidates the buffers that overflowed, else those past the high-water mark
            const int counts = lane < QT ? s_cnt[lane] : 0;   // one LDS read for the wave's sixteen (eight) queries
            for (int ql = wave; ql < QT; ql += kKnnWaves) {
                const int seen = __builtin_amdgcn_readlane(counts, ql);
                const int n = seen < cap ? seen : cap;
                if (any ? seen <= cap : n <= (k + cap) / 2) continue;   // (without pending candidates seen <= cap)
                unsigned long long* buf = s_buf + ql * cap;
                unsigned long long e[NG];
                int r[NG];
#pragma unroll
                for (int j = 0; j < NG; ++j) e[j] = lane + 64 * j < n ? buf[lane + 64 * j] : kKnnNone;
                knn_ranks<NG>(e, n, r);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int j = 0; j < NG; ++j)
                    if (lane + 64 * j < n && r[j] < k) buf[r[j]] = e[j];
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) { s_cnt[ql] = n < k ? n : k; s_thr[ql] = n >= k ? buf[k - 1] : kKnnNone; }
            }
            __syncthreads();
            if (!any) break;
        }
#pragma unroll
        for (int ni = 0; ni < NQ; ++ni) acc[ni] = f32x16{0};
    }

    // ---- the slab's k best pairs of every query, sorted; places behind them hold MAX
    for (int ql = wave; ql < QT; ql += kKnnWaves) {
        const int64_t q = q0 + ql;
        if (q >= nq) break;
        const int n = __builtin_amdgcn_readfirstlane(s_cnt[ql]);       // <= cap: every step leaves it so
        unsigned long long* buf = s_buf + ql * cap;
        unsigned long long e[NG];
        int r[NG];
#pragma unroll
        for (int j = 0; j < NG; ++j) e[j] = lane + 64 * j < n ? buf[lane + 64 * j] : kKnnNone;
        knn_ranks<NG>(e, n, r);
        unsigned long long* out = part + ((size_t)q * S + sp) * k;
#pragma unroll
        for (int j = 0; j < NG; ++j)
            if (lane + 64 * j < n && r[j] < k) out[r[j]] = e[j];
        for (int j = (n < k ? n : k) + lane; j < k; j += 64) out[j] = kKnnNone;
    }
}

__global__ void __launch_bounds__(kKnnBlock) k_knn_finish(const unsigned long long* __restrict__ part, int n_in, int P, int k, int metric,
                                                            const float* __restrict__ table, int64_t table_stride,
                                                            const float* __restrict__ queries, int64_t query_stride, int dim,
                                                            int32_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                            int32_t* __restrict__ out_count) {
    __shared__ unsigned long long s_pair[kKnnFinishMax];
    __shared__ unsigned long long s_dist[KGE_KNN_MAX];
    __shared__ int s_live;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const unsigned long long* __restrict__ in = part + (size_t)q * n_in;
    if (tid == 0) s_live = 0;
    for (int j = tid; j < P; j += kKnnBlock) s_pair[j] = j < n_in ? in[j] : kKnnNone;
    __syncthreads();
    auto sort = [&](unsigned long long* a, int n) {
        for (int size = 2; size <= n; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (n >> 1); t += kKnnBlock) {
                    const int x = 2 * t - (t & (stride - 1)), y = x + stride;
                    const unsigned long long vx = a[x], vy = a[y];
                    if ((vx > vy) == ((x & size) == 0)) { a[x] = vy; a[y] = vx; }
                }
                __syncthreads();
            }
    };
    sort(s_pair, P);
    // live places: the pairs sort before the MAX padding
    if (tid < k && tid < P && s_pair[tid] != kKnnNone) atomicAdd(&s_live, 1);
    __syncthreads();
    const int kk = s_live;
    const unsigned long long* res = s_pair;
    if (metric == KGE_KNN_L2) {
        int P2 = 1;
        while (P2 < k) P2 <<= 1;
        const float* __restrict__ qrow = queries + q * query_stride;
        for (int j = wave; j < P2; j += kKnnWaves) {
            unsigned long long p = kKnnNone;
            if (j < kk) {
                const uint32_t id = (uint32_t)s_pair[j];
                const float* __restrict__ crow = table + (int64_t)id * table_stride;
                float s = 0.f;
                for (int i = lane; i < dim; i += 64) { const float d = qrow[i] - crow[i]; s = fmaf(d, d, s); }
                s = sqrtf(knn_wave_sum(s));
                p = ((unsigned long long)knn_key(s, false) << 32) | id;
            }
            if (lane == 0) s_dist[j] = p;
        }
        __syncthreads();
        sort(s_dist, P2);
        res = s_dist;
    }
    for (int j = tid; j < k; j += kKnnBlock) {
        int32_t id = -1;
        float sc = __uint_as_float(0x7fc00000u);
        if (j < kk) { id = (int32_t)(uint32_t)res[j]; sc = knn_unkey((uint32_t)(res[j] >> 32), metric != KGE_KNN_L2); }
        out_ids[q * k + j] = id;
        out_scores[q * k + j] = sc;
    }
    if (tid == 0) out_count[q] = kk;
}

namespace {

struct KnnPlan { int nqb; int cap; int64_t qtiles, ctiles, tiles_per; int S; size_t norm_bytes, bytes; };

// The candidate split: enough slabs that one query tile still fills the device, at most what k_knn_finish sorts in LDS; KGE_KNN_SPLIT
// forces it.  Slabs are whole steps of 128 candidates and none is empty.
KnnPlan knn_plan(int64_t nq, int64_t n_rows, int32_t k, int metric) {
    KnnPlan p;
    p.nqb = k <= 32 ? 2 : 1;                            // 64 queries per tile while their buffers fit one wave: 64 places each
    p.cap = p.nqb == 2 ? 64 : k + kKnnExtra;            // at most 160: three places per lane
    const int qt = 32 * p.nqb;
    p.qtiles = (nq + qt - 1) / qt;
    p.ctiles = (n_rows + kKnnCT - 1) / kKnnCT;
    int64_t most = kKnnFinishMax / k;
    if (most > 64) most = 64;
    if (most > p.ctiles) most = p.ctiles;
    int64_t want = switch_value("KNN_SPLIT");
    if (want < 1) want = p.qtiles > 0 ? kKnnTargetGroups / p.qtiles : 1;   // rounded down: one residency round, not one and a bit
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.tiles_per = (p.ctiles + want - 1) / want;
    p.S = (int)((p.ctiles + p.tiles_per - 1) / p.tiles_per);
    p.norm_bytes = metric == KGE_KNN_DOT ? 0 : align256((size_t)n_rows * sizeof(float)) + align256((size_t)nq * sizeof(float));
    p.bytes = p.norm_bytes + align256((size_t)nq * p.S * k * sizeof(unsigned long long)) + 256;   // + 256: the pointer is aligned up
    return p;
}

const char* knn_check(const char* who, int64_t nq, int64_t n_rows, int64_t dim, int32_t k, int metric) {
    static thread_local char msg[160];
    if (k < 1 || k > KGE_KNN_MAX) { snprintf(msg, sizeof msg, "%s: k = %d outside 1..%d (KGE_KNN_MAX)", who, (int)k, KGE_KNN_MAX); return msg; }
    if (metric < KGE_KNN_DOT || metric > KGE_KNN_L2) { snprintf(msg, sizeof msg, "%s: metric = %d (0 = dot, 1 = cosine, 2 = l2)", who, metric); return msg; }
    if (dim < 1 || dim > 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: dim = %lld outside 1..2^31-1", who, (long long)dim); return msg; }
    if (n_rows < 1 || n_rows > 0x7fffff00ll) { snprintf(msg, sizeof msg, "%s: n_rows = %lld outside 1..2^31-257 (candidate ids are int32)", who, (long long)n_rows); return msg; }
    if (nq < 0 || nq > 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: nq = %lld outside 0..2^31-1", who, (long long)nq); return msg; }
    return nullptr;
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_knn_workspace_bytes(int64_t nq, int64_t n_rows, int64_t dim, int32_t k, int metric) {
    if (knn_check("kge_knn_workspace_bytes", nq, n_rows, dim, k, metric) || nq == 0) return 0;
    return knn_plan(nq, n_rows, k, metric).bytes;
}

int kge_knn_rows(const float* table, int64_t n_rows, int64_t dim, int64_t table_stride, const float* queries, int64_t nq,
                 int64_t query_stride, const int64_t* self_ids, int32_t k, int metric, void* workspace, size_t workspace_bytes,
                 int32_t* out_ids, float* out_scores, int32_t* out_count, void* stream) {
    const char* who = "kge_knn_rows";
    if (const char* bad = knn_check(who, nq, n_rows, dim, k, metric)) { set_error("%s", bad); return -1; }
    if (table_stride < dim) { set_error("%s: table_stride = %lld < dim = %lld", who, (long long)table_stride, (long long)dim); return -1; }
    if (query_stride < dim) { set_error("%s: query_stride = %lld < dim = %lld", who, (long long)query_stride, (long long)dim); return -1; }
    if (!table || !queries || !out_ids || !out_scores || !out_count) {
        set_error("%s: null table / queries / out_ids / out_scores / out_count", who);
        return -1;
    }
    if (nq == 0) return 0;
    const KnnPlan p = knn_plan(nq, n_rows, k, metric);
    if (!workspace || workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_knn_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p.bytes);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* tnorm = nullptr;
    float* qnorm = nullptr;
    if (metric != KGE_KNN_DOT) {
        tnorm = (float*)base;
        qnorm = (float*)(base + align256((size_t)n_rows * sizeof(float)));
        hipLaunchKernelGGL(k_knn_norms, dim3((unsigned)((n_rows + nq + kKnnWaves - 1) / kKnnWaves)), dim3(kKnnBlock), 0, s, table, n_rows,
                           table_stride, queries, nq, query_stride, (int)dim, metric == KGE_KNN_COSINE ? 1 : 0, tnorm, qnorm);
        if (int rc = check_launch("k_knn_norms")) return rc;
    }
    unsigned long long* part = (unsigned long long*)(base + p.norm_bytes);
    const dim3 grid((unsigned)p.qtiles, (unsigned)p.S);
    const size_t lds = knn_sweep_lds(32 * p.nqb, p.cap);
#define KGE_KNN_SWEEP(NQ, METRIC)                                                                                                  \
    hipLaunchKernelGGL((k_knn_sweep<NQ, METRIC>), grid, dim3(kKnnBlock), lds, s, table, n_rows, (int)dim, table_stride, queries, nq, \
                       query_stride, self_ids, (int)k, p.cap, (int)p.tiles_per, (int)p.ctiles, tnorm, qnorm, part)
    if (p.nqb == 2) {
        if (metric == KGE_KNN_DOT) KGE_KNN_SWEEP(2, KGE_KNN_DOT);
        else if (metric == KGE_KNN_COSINE) KGE_KNN_SWEEP(2, KGE_KNN_COSINE);
        else KGE_KNN_SWEEP(2, KGE_KNN_L2);
    } else {
        if (metric == KGE_KNN_DOT) KGE_KNN_SWEEP(1, KGE_KNN_DOT);
        else if (metric == KGE_KNN_COSINE) KGE_KNN_SWEEP(1, KGE_KNN_COSINE);
        else KGE_KNN_SWEEP(1, KGE_KNN_L2);
    }
#undef KGE_KNN_SWEEP
    if (int rc = check_launch("k_knn_sweep")) return rc;
    const int n_in = p.S * (int)k;
    int P = 1;
    while (P < n_in) P <<= 1;
    hipLaunchKernelGGL(k_knn_finish, dim3((unsigned)nq), dim3(kKnnBlock), 0, s, part, n_in, P, (int)k, metric, table, table_stride, queries,
                       query_stride, (int)dim, out_ids, out_scores, out_count);
    return check_launch("k_knn_finish");
}

}  // extern "C"
