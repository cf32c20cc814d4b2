// kge_silhouette.hip -- silhouette scores (Rousseeuw 1987) of labelled embedding rows: an all-pairs quantity computed without an
// [n, n] distance block, without float atomics, every sum in a fixed order -- a deterministic function of (rows, label).
//
//   k_sil_rows          one wave per row: |x|^2 in float32 (lanes stride the row, xor butterfly), and the row's effective label: -1 for
//                       a row with a NaN entry or a label outside 0..k-1 -- such a row is in no cluster and is no column of the sweep.
//   k_sil_hist / _scan / _scatter    effective labels -> the member list, ordered by cluster, ascending row id inside a cluster, every
//                       cluster padded with -1 to whole tiles of 32 columns: the counting sort of kge_kmeans.hip (rank inside blocks of
//                       1024 rows, one scan, plain stores).  The scan also writes the counts, the padding, and the S + 1 slab cuts
//                       (tile indices on cluster boundaries); the scatter also writes the cluster of every tile.
//   k_sil_sweep         a workgroup of 4 waves owns 128 rows and one slab of column tiles; each wave owns 32 of the rows for the whole
//                       sweep.  A step is 4 column tiles (128 member slots), gathered through the member list into k-major LDS slabs of
//                       32 dims that the waves share; the wave's rows are the B operand of mfma_f32_32x32x2f32, a column tile the A
//                       operand, four accumulator blocks per wave (5 LDS reads feed 4 matrix instructions).  The next fill's operands
//                       wait in registers (unconditional loads from clamped addresses, zeroed at the LDS store).  After the last dim slab
//                       a lane holds 16 distances of ONE row per tile, lane ^ 32 the other 16: d is formed, the self column and the
//                       padding are masked by index, 16 terms are added in float32 in register order, then the two halves, and the tile
//                       sum joins the float64 running sum of the tile's cluster.  When the cluster changes the segment closes: into
//                       S_own, or as a mean into the running (least mean, its cluster).  No sum ever crosses a wave.
//   k_sil_finish        one thread per row folds the S slab partials -- at most one S_own, the least (mean, id) -- into a, b, s and the
//                       neighbour, all in float64, rounded once.
//   k_sil_score         one workgroup: thread t adds out_s of rows t, t + 1024, ... in float64, then a tree over the threads.
#include <cstdio>
#include "kge_internal.h"

namespace kge {

namespace {

constexpr int kSilBlock = 256;
constexpr int kSilWaves = kSilBlock / 64;
constexpr int kSilRT = 32 * kSilWaves;     // rows of a workgroup
constexpr int kSilTile = 32;               // columns of a tile: one cluster each
constexpr int kSilStepTiles = 4;
constexpr int kSilCT = kSilTile * kSilStepTiles;   // member slots per step
constexpr int kSilKS = 32;                 // dim slab of one LDS fill
constexpr int kSilCS = kSilCT + 4;         // k-major operand rows, padded
constexpr int kSilQS = kSilRT + 4;
constexpr int kSilGroupRows = 1024;        // rows per block of the counting sort
constexpr int kSilScanBlock = 1024;
constexpr int kSilMaxSplit = 64;
constexpr int kSilTargetGroups = 256;      // one workgroup on each of 256 compute units (300 registers: one wave per SIMD)

}  // namespace

__global__ void __launch_bounds__(kSilBlock) k_sil_rows(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                         const int32_t* __restrict__ label, int k, float* __restrict__ norm,
                                                         int32_t* __restrict__ eff) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kSilWaves + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* __restrict__ src = rows + i * row_stride;
    float s = 0.f;
    bool bad = false;
    for (int j = lane; j < dim; j += 64) { const float v = src[j]; bad |= v != v; s = fmaf(v, v, s); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    const bool nan = __ballot(bad) != 0ull;
    if (lane == 0) {
        const int lab = label[i];
        norm[i] = s;
        eff[i] = (nan || lab < 0 || lab >= k) ? -1 : lab;
    }
}

// block b ranks rows [1024 b, 1024 b + 1024): rank[i] = rows of the block before i with i's label; hist[b][c] = the block's rows of c
__global__ void __launch_bounds__(kSilBlock) k_sil_hist(const int32_t* __restrict__ eff, int64_t n, int k, int32_t* __restrict__ rank,
                                                         int32_t* __restrict__ hist) {
    __shared__ int s_hist[KGE_KMEANS_MAX_K];
    __shared__ int s_lab[kSilBlock];
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += kSilBlock) s_hist[c] = 0;
    for (int p = 0; p < kSilGroupRows / kSilBlock; ++p) {
        const int64_t i = (int64_t)blockIdx.x * kSilGroupRows + p * kSilBlock + tid;
        const int lab = i < n ? eff[i] : -1;
        __syncthreads();
        s_lab[tid] = lab;
        __syncthreads();
        int before = 0, after = 0;
        if (lab >= 0) {
            for (int t = 0; t < kSilBlock; ++t) {
                const int same = s_lab[t] == lab ? 1 : 0;
                before += t < tid ? same : 0;
                after += t > tid ? same : 0;
            }
            rank[i] = s_hist[lab] + before;
        }
        __syncthreads();
        if (lab >= 0 && after == 0) s_hist[lab] += before + 1;   // the label's last row of the pass: one writer per label
    }
    __syncthreads();
    for (int c = tid; c < k; c += kSilBlock) hist[(size_t)blockIdx.x * k + c] = s_hist[c];
}

// One workgroup.  hist[b][c] -> the rows of c in the blocks before b; count[c]; poff[c]: first slot of cluster c in the padded member
// list ([k + 1], multiples of 32); the -1 padding behind every cluster's members; cut[s], s = 0..S: the first tile of slab s -- the
// first cluster boundary at or behind tile floor(T s / S), T the number of tiles.
__global__ void __launch_bounds__(kSilScanBlock) k_sil_scan(int32_t* __restrict__ hist, int64_t nb, int k, int S, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ poff, int32_t* __restrict__ members,
                                                             int32_t* __restrict__ cut) {
    constexpr int PER = KGE_KMEANS_MAX_K / kSilScanBlock;
    __shared__ int s_cnt[KGE_KMEANS_MAX_K];
    __shared__ int s_off[KGE_KMEANS_MAX_K + 1];
    __shared__ int s_a[kSilScanBlock];
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += kSilScanBlock) {
        int run = 0;
        for (int64_t b = 0; b < nb; ++b) { const int v = hist[b * k + c]; hist[b * k + c] = run; run += v; }
        s_cnt[c] = run;
        count[c] = run;
    }
    __syncthreads();
    int mine = 0;
    for (int j = 0; j < PER; ++j) {
        const int c = tid * PER + j;
        mine += c < k ? (s_cnt[c] + kSilTile - 1) / kSilTile * kSilTile : 0;
    }
    s_a[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kSilScanBlock; d <<= 1) {
        const int a = tid >= d ? s_a[tid - d] : 0;
        __syncthreads();
        s_a[tid] += a;
        __syncthreads();
    }
    int run = s_a[tid] - mine;
    for (int j = 0; j < PER; ++j) {
        const int c = tid * PER + j;
        if (c < k) {
            const int cnt = s_cnt[c], pad = (cnt + kSilTile - 1) / kSilTile * kSilTile;
            s_off[c] = run;
            poff[c] = run;
            for (int p = cnt; p < pad; ++p) members[run + p] = -1;
            run += pad;
        }
    }
    const int total = s_a[kSilScanBlock - 1];
    if (tid == 0) { s_off[k] = total; poff[k] = total; }
    __syncthreads();
    if (tid <= S) {
        const int target = (int)((int64_t)(total / kSilTile) * tid / S) * kSilTile;
        int lo = -1, hi = k;   // the lowest c with s_off[c] >= target: s_off[k] is the total
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] >= target) hi = mid; else lo = mid; }
        cut[tid] = s_off[hi] / kSilTile;
    }
}

__global__ void __launch_bounds__(kSilBlock) k_sil_scatter(const int32_t* __restrict__ eff, int64_t n, int k, const int32_t* __restrict__ rank,
                                                            const int32_t* __restrict__ hist, const int32_t* __restrict__ poff,
                                                            int32_t* __restrict__ members, int32_t* __restrict__ tile_cl) {
    const int64_t i = (int64_t)blockIdx.x * kSilBlock + threadIdx.x;
    if (i >= n) return;
    const int lab = eff[i];
    if (lab < 0) return;
    const int pos = poff[lab] + hist[(i / kSilGroupRows) * k + lab] + rank[i];
    members[pos] = (int32_t)i;
    if ((pos & (kSilTile - 1)) == 0) tile_cl[pos / kSilTile] = lab;
}

template <bool COS>
__global__ void __launch_bounds__(kSilBlock) k_sil_sweep(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                          const float* __restrict__ norm, const int32_t* __restrict__ eff,
                                                          const int32_t* __restrict__ members, const int32_t* __restrict__ tile_cl,
                                                          const int32_t* __restrict__ cut, const int32_t* __restrict__ count,
                                                          double* __restrict__ part /* [2][S][n] own, best */,
                                                          int32_t* __restrict__ p_id) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    __shared__ float sC[kSilKS * kSilCS];
    __shared__ float sQ[kSilKS * kSilQS];
    __shared__ int2 s_col[2][kSilCT];   // (member id or -1, the bits of its |x|^2) of the step's slots, by step parity

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, lk = lane >> 5;
    const int q0 = blockIdx.x * kSilRT;   // (row ids are int32)
    const int t0 = cut[blockIdx.y], t1 = cut[blockIdx.y + 1];
    const int steps = (t1 - t0 + kSilStepTiles - 1) / kSilStepTiles;
    const int nslab = (dim - 1) / kSilKS + 1;
    const int n_rows = (int)n;
    const int q_last = (n_rows - 1 - q0 < kSilRT - 1) ? n_rows - 1 - q0 : kSilRT - 1;   // the tile's last row (n > q0: the grid covers n)
    const int my_row = q0 + wave * 32 + li;
    const int my_rc = my_row < n_rows ? my_row : n_rows - 1;
    const int my_lab = eff[my_rc];
    const float xn = norm[my_rc];

    // global -> registers -> LDS, one fill ahead of the matrix cores: unconditional loads from addresses clamped into the tables, what
    // is a zero (a padding slot, past the slab, n or dim) is remembered in a bit mask and applied at the LDS store
    float rc[16], rq[16];
    const float* cp[16];   // the member rows of the step in flight and the workgroup's rows: per-lane pointers, kept in vector
    const float* qp[16];   // registers (left to itself the compiler keeps 30 scalar row offsets and spills scalar registers)
    int col_m = -1;
    float col_n = 0.f;
    uint32_t row_ok = 0, ld_ok = 0;   // bit i: cp[i] is a member row, bit 16 + i: qp[i] is a row below n; ld_ok: those inside dim
    int ld_t = 0, ld_s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ql = (tid >> 5) + 8 * i;
        const bool in = ql <= q_last;
        qp[i] = rows + (int64_t)(q0 + (in ? ql : q_last)) * row_stride;
        asm volatile("" : "+v"(qp[i]));
        row_ok |= in ? 65536u << i : 0u;
    }
    auto load_step = [&]() __attribute__((always_inline)) {
        if (ld_s == 0) {   // a new step: its member ids
            const int base = (t0 + ld_t * kSilStepTiles) * kSilTile, lim = t1 * kSilTile;   // (slots are below 2^31)
            row_ok &= 0xffff0000u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = base + (tid >> 5) + 8 * i;
                const int m = members[j < lim ? j : lim - 1];
                const bool in = j < lim && m >= 0;
                cp[i] = rows + (int64_t)(in ? m : 0) * row_stride;
                asm volatile("" : "+v"(cp[i]));
                row_ok |= in ? 1u << i : 0u;
            }
            if (tid < kSilCT) {
                const int j = base + tid;
                const int m = members[j < lim ? j : lim - 1];
                col_m = j < lim ? m : -1;
                col_n = norm[col_m < 0 ? 0 : col_m];
            }
        }
        const int kd = ld_s * kSilKS + (tid & 31);
        const bool kin = kd < dim;
        const int kc = kin ? kd : dim - 1;
        ld_ok = kin ? row_ok : 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) rc[i] = cp[i][kc];
#pragma unroll
        for (int i = 0; i < 16; ++i) rq[i] = qp[i][kc];
        if (++ld_s == nslab) { ld_s = 0; ++ld_t; }
    };

    // the row's state: identical in both lane halves
    double run = 0.0, own = -1.0, best = 0.0;   // own < 0: the row's cluster is not in this slab
    int cur = -1, bid = -1;
    auto close = [&]() __attribute__((always_inline)) {
        if (cur < 0) return;
        if (cur == my_lab) own = run;
        else {
            const double mean = run / (double)count[cur];
            if (bid < 0 || mean < best) { best = mean; bid = cur; }   // clusters arrive in ascending id: the lower id keeps a tie
        }
    };

    f32x16 acc[kSilStepTiles];
#pragma unroll
    for (int ct = 0; ct < kSilStepTiles; ++ct) acc[ct] = f32x16{0};
    if (steps > 0) load_step();
    for (int st = 0; st < steps; ++st) {
        for (int sl = 0; sl < nslab; ++sl) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sC[(tid & 31) * kSilCS + (tid >> 5) + 8 * i] = (ld_ok >> i) & 1u ? rc[i] : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sQ[(tid & 31) * kSilQS + (tid >> 5) + 8 * i] = (ld_ok >> (16 + i)) & 1u ? rq[i] : 0.f;
            if (sl == 0 && tid < kSilCT) s_col[st & 1][tid] = make_int2(col_m, (int)__float_as_uint(col_n));
            __syncthreads();
            if (ld_t < steps) load_step();
#pragma unroll
            for (int kk = 0; kk < kSilKS; kk += 2) {
                const float b = sQ[(kk + lk) * kSilQS + wave * 32 + li];
#pragma unroll
                for (int ct = 0; ct < kSilStepTiles; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(sC[(kk + lk) * kSilCS + ct * 32 + li], b, acc[ct], 0, 0, 0);
            }
            __syncthreads();   // the slab is consumed: the next fill may overwrite it
        }
        // ---- the step's products are complete: the lane owns row li of its wave, register r of block ct is slot
        // ct * 32 + (r & 3) + 8 (r >> 2) + 4 lk of the step
#pragma unroll
        for (int ct = 0; ct < kSilStepTiles; ++ct) {
            const int tile = t0 + st * kSilStepTiles + ct;
            if (tile < t1) {
                const int c = tile_cl[tile];
                if (c != cur) { close(); cur = c; run = 0.0; }
                float t = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int2 col = s_col[st & 1][ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk];
                    float d;
                    if (COS) d = fmaxf(1.0f - acc[ct][r], 0.f);
                    else d = __fsqrt_rn(fmaxf((xn + __uint_as_float((uint32_t)col.y)) - 2.0f * acc[ct][r], 0.f));
                    t += (col.x < 0 || col.x == my_row) ? 0.f : d;
                }
                t += __shfl_xor(t, 32);
                run += (double)t;
            }
            acc[ct] = f32x16{0};
        }
    }
    close();
    if (lk == 0 && my_row < n_rows) {
        const size_t at = (size_t)blockIdx.y * (size_t)n + (size_t)my_row;
        part[at] = own;
        part[(size_t)gridDim.y * (size_t)n + at] = best;
        p_id[at] = bid;
    }
}

__global__ void __launch_bounds__(kSilBlock) k_sil_finish(int64_t n, int S, const int32_t* __restrict__ eff, const int32_t* __restrict__ count,
                                                           const double* __restrict__ p_own, const double* __restrict__ p_best,
                                                           const int32_t* __restrict__ p_id, float* __restrict__ out_s,
                                                           float* __restrict__ out_a, float* __restrict__ out_b,
                                                           int32_t* __restrict__ out_neighbor) {
    const int64_t i = (int64_t)blockIdx.x * kSilBlock + threadIdx.x;
    if (i >= n) return;
    const float qnan = __uint_as_float(0x7fc00000u);
    const int lab = eff[i];
    if (lab < 0) { out_s[i] = qnan; out_a[i] = qnan; out_b[i] = qnan; out_neighbor[i] = -1; return; }
    double own = 0.0, best = 0.0;
    int bid = -1;
    for (int s = 0; s < S; ++s) {   // slabs hold ascending clusters: the earlier slab keeps a tie
        const size_t at = (size_t)s * (size_t)n + (size_t)i;
        const double o = p_own[at], m = p_best[at];
        const int id = p_id[at];
        if (o >= 0.0) own = o;
        if (id >= 0 && (bid < 0 || m < best)) { best = m; bid = id; }
    }
    const int cnt = count[lab];
    const double a = cnt > 1 ? own / (double)(cnt - 1) : 0.0;
    const double hi = a > best ? a : best;
    double s = 0.0;
    if (cnt > 1 && bid >= 0 && hi > 0.0) s = (best - a) / hi;
    out_s[i] = (float)s;
    out_a[i] = (float)a;
    out_b[i] = bid >= 0 ? (float)best : qnan;
    out_neighbor[i] = bid;
}

__global__ void __launch_bounds__(kSilScanBlock) k_sil_score(int64_t n, const int32_t* __restrict__ eff, const float* __restrict__ out_s,
                                                              double* __restrict__ out_score) {
    __shared__ double s_sum[kSilScanBlock];
    __shared__ long long s_num[kSilScanBlock];
    const int tid = threadIdx.x;
    double s = 0.0;
    long long num = 0;
    for (int64_t i = tid; i < n; i += kSilScanBlock)
        if (eff[i] >= 0) { s += (double)out_s[i]; ++num; }
    s_sum[tid] = s;
    s_num[tid] = num;
    __syncthreads();
    for (int d = kSilScanBlock / 2; d > 0; d >>= 1) {
        if (tid < d) { s_sum[tid] += s_sum[tid + d]; s_num[tid] += s_num[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) out_score[0] = s_num[0] > 0 ? s_sum[0] / (double)s_num[0] : __longlong_as_double(0x7ff8000000000000ll);
}

namespace {

struct SilPlan {
    int64_t nb, slots, tiles, rtiles;
    int S;
    size_t o_norm, o_eff, o_rank, o_hist, o_poff, o_members, o_tile, o_cut, o_own, o_id, bytes;
};

// The column split is a function of n alone: enough slabs that the row tiles fill the device; KGE_SIL_SPLIT forces it
SilPlan sil_plan(int64_t n, int32_t k) {
    SilPlan p;
    p.nb = (n + kSilGroupRows - 1) / kSilGroupRows;
    p.slots = (n + (int64_t)(kSilTile - 1) * k + kSilTile - 1) / kSilTile * kSilTile;   // the padded member list stays below
    p.tiles = p.slots / kSilTile;
    p.rtiles = (n + kSilRT - 1) / kSilRT;
    int64_t want = switch_value("SIL_SPLIT");
    if (want < 1) want = kSilTargetGroups / p.rtiles;
    if (want > kSilMaxSplit) want = kSilMaxSplit;
    if (want < 1) want = 1;
    p.S = (int)want;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    p.o_norm = take((size_t)n * sizeof(float));
    p.o_eff = take((size_t)n * sizeof(int32_t));
    p.o_rank = take((size_t)n * sizeof(int32_t));
    p.o_hist = take((size_t)p.nb * k * sizeof(int32_t));
    p.o_poff = take((size_t)(k + 1) * sizeof(int32_t));
    p.o_members = take((size_t)p.slots * sizeof(int32_t));
    p.o_tile = take((size_t)p.tiles * sizeof(int32_t));
    p.o_cut = take((size_t)(p.S + 1) * sizeof(int32_t));
    p.o_own = take((size_t)2 * p.S * n * sizeof(double));   // [S][n] own sums, then [S][n] least means
    p.o_id = take((size_t)p.S * n * sizeof(int32_t));
    p.bytes = o + 256;   // + 256: the pointer is aligned up
    return p;
}

const char* sil_check(const char* who, int64_t n, int64_t dim, int64_t k, int metric) {
    static thread_local char msg[200];
    if (n < 2 || n > 0x7ffe0000ll) { snprintf(msg, sizeof msg, "%s: n = %lld outside 2..2^31-2^17 (row ids are int32)", who, (long long)n); return msg; }
    if (dim < 1 || dim > 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: dim = %lld outside 1..2^31-1", who, (long long)dim); return msg; }
    if (k < 2 || k > KGE_KMEANS_MAX_K) { snprintf(msg, sizeof msg, "%s: k = %lld outside 2..KGE_KMEANS_MAX_K = %d", who, (long long)k, KGE_KMEANS_MAX_K); return msg; }
    if (metric != KGE_SIL_L2 && metric != KGE_SIL_COSINE) { snprintf(msg, sizeof msg, "%s: metric = %d (0 = l2, 1 = cosine)", who, metric); return msg; }
    return nullptr;
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_silhouette_workspace_bytes(int64_t n, int64_t dim, int32_t k) {
    if (sil_check("kge_silhouette_workspace_bytes", n, dim, k, KGE_SIL_L2)) return 0;
    return sil_plan(n, k).bytes;
}

int kge_silhouette(const float* rows, int64_t n, int64_t dim, int64_t row_stride, const int32_t* label, int32_t k, int metric,
                   void* workspace, size_t workspace_bytes, float* out_s, float* out_a, float* out_b, int32_t* out_neighbor,
                   int32_t* out_count, double* out_score, void* stream) {
    const char* who = "kge_silhouette";
    if (const char* bad = sil_check(who, n, dim, k, metric)) { set_error("%s", bad); return -1; }
    if (row_stride < dim) { set_error("%s: row_stride = %lld < dim = %lld", who, (long long)row_stride, (long long)dim); return -1; }
    if (!rows || !label || !out_s || !out_a || !out_b || !out_neighbor || !out_count || !out_score) {
        set_error("%s: null rows / label / out_s / out_a / out_b / out_neighbor / out_count / out_score", who);
        return -1;
    }
    const SilPlan p = sil_plan(n, k);
    if (!workspace || workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_silhouette_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p.bytes);
        return -1;
    }
    char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* norm = (float*)(base + p.o_norm);
    int32_t* eff = (int32_t*)(base + p.o_eff);
    int32_t* rank = (int32_t*)(base + p.o_rank);
    int32_t* hist = (int32_t*)(base + p.o_hist);
    int32_t* poff = (int32_t*)(base + p.o_poff);
    int32_t* members = (int32_t*)(base + p.o_members);
    int32_t* tile_cl = (int32_t*)(base + p.o_tile);
    int32_t* cut = (int32_t*)(base + p.o_cut);
    double* p_own = (double*)(base + p.o_own);
    double* p_best = p_own + (size_t)p.S * n;
    int32_t* p_id = (int32_t*)(base + p.o_id);
    hipStream_t s = (hipStream_t)stream;
    const unsigned row_blocks = (unsigned)((n + kSilBlock - 1) / kSilBlock);

    hipLaunchKernelGGL(k_sil_rows, dim3((unsigned)((n + kSilWaves - 1) / kSilWaves)), dim3(kSilBlock), 0, s, rows, n, (int)dim, row_stride,
                       label, (int)k, norm, eff);
    if (int rc = check_launch("k_sil_rows")) return rc;
    hipLaunchKernelGGL(k_sil_hist, dim3((unsigned)p.nb), dim3(kSilBlock), 0, s, (const int32_t*)eff, n, (int)k, rank, hist);
    if (int rc = check_launch("k_sil_hist")) return rc;
    hipLaunchKernelGGL(k_sil_scan, dim3(1), dim3(kSilScanBlock), 0, s, hist, p.nb, (int)k, p.S, out_count, poff, members, cut);
    if (int rc = check_launch("k_sil_scan")) return rc;
    hipLaunchKernelGGL(k_sil_scatter, dim3(row_blocks), dim3(kSilBlock), 0, s, (const int32_t*)eff, n, (int)k, (const int32_t*)rank,
                       (const int32_t*)hist, (const int32_t*)poff, members, tile_cl);
    if (int rc = check_launch("k_sil_scatter")) return rc;
    const dim3 grid((unsigned)p.rtiles, (unsigned)p.S);
    if (metric == KGE_SIL_COSINE)
        hipLaunchKernelGGL((k_sil_sweep<true>), grid, dim3(kSilBlock), 0, s, rows, n, (int)dim, row_stride, (const float*)norm,
                           (const int32_t*)eff, (const int32_t*)members, (const int32_t*)tile_cl, (const int32_t*)cut,
                           (const int32_t*)out_count, p_own, p_id);
    else
        hipLaunchKernelGGL((k_sil_sweep<false>), grid, dim3(kSilBlock), 0, s, rows, n, (int)dim, row_stride, (const float*)norm,
                           (const int32_t*)eff, (const int32_t*)members, (const int32_t*)tile_cl, (const int32_t*)cut,
                           (const int32_t*)out_count, p_own, p_id);
    if (int rc = check_launch("k_sil_sweep")) return rc;
    hipLaunchKernelGGL(k_sil_finish, dim3(row_blocks), dim3(kSilBlock), 0, s, n, p.S, (const int32_t*)eff, (const int32_t*)out_count,
                       (const double*)p_own, (const double*)p_best, (const int32_t*)p_id, out_s, out_a, out_b, out_neighbor);
    if (int rc = check_launch("k_sil_finish")) return rc;
    hipLaunchKernelGGL(k_sil_score, dim3(1), dim3(kSilScanBlock), 0, s, n, (const int32_t*)eff, (const float*)out_s, out_score);
    return check_launch("k_sil_score");
}

}  // extern "C"
