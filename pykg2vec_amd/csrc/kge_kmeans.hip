// kge_kmeans.hip -- k-means clustering of embedding rows (Lloyd's iteration and the k-means++ seeding), a deterministic function of its
// inputs: no [n, k] distance block is written, no float atomic is used, every sum runs in a fixed order.
//
//   k_kmeans_cnorm      |c|^2 of every centroid: one wave per centroid, lanes stride the row, xor butterfly -- a fixed order.
//   k_kmeans_assign     a workgroup of 4 waves owns a tile of 64 (32 at small n) rows and walks ALL centroids, 128 per step, on
//                       mfma_f32_32x32x2f32: centroids on the A side, rows on the B side, operands through k-major LDS slabs of 32
//                       columns (the arrangement of k_knn_sweep), the next step's operands in registers while this one runs.  A lane
//                       owns one row; its 16 accumulators are centroid rows.  key = |c|^2 - 2 x.c becomes the ascending unsigned key
//                       of the project's total order and the pair (key << 32 | id) is compared with the lane's running best: two
//                       registers, no list, no vote.  The eight partial winners of a row (4 waves x 2 lane halves) meet in LDS -- the
//                       minimum of a total order needs no combine order --, then one wave per row recomputes the squared distance to
//                       the winner directly, finds the rows with a NaN entry (label -1) and counts the labels that changed.
//   k_kmeans_hist / _scan / _scatter    labels -> member lists in ascending row id per cluster: a counting sort.  A block of 1024 rows
//                       ranks its rows among the earlier rows of the block with the same label and writes its histogram; one
//                       workgroup scans the histograms over blocks and clusters (and, inside kge_kmeans_run, sums the inertia in
//                       float64 and keeps the run's state); the scatter is then a plain store per row: stable, no atomics.
//   k_kmeans_update     one wave owns one chunk of KGE_KMEANS_CHUNK members of one cluster and 64 columns: float32 sums in member order.
//   k_kmeans_finish     one workgroup per cluster: chunk sums added in chunk order in float64, the mean (divided by its float64 norm
//                       under unit_centroids), rounded to float32 once.
//   k_kmeans_seed_fold / _pick    k-means++: fold the newest centre into every row's running minimum and write block sums; scan the
//                       block sums in float64 in order and pick the first row whose prefix passes u[j] T.
// The only atomics are integer adds / minima whose results do not depend on the order (counts, a lowest index).
#include <cstdio>
#include <climits>
#include "kge_internal.h"

namespace kge {

namespace {

constexpr int kKmBlock = 256;
constexpr int kKmWaves = kKmBlock / 64;
constexpr int kKmCT = 128;               // centroids per step: 32 per wave
constexpr int kKmKS = 32;                // dim slab of one LDS fill
constexpr int kKmCS = kKmCT + 4;         // k-major operand rows, padded
constexpr int kKmGroupRows = 1024;       // rows per block of the counting sort
constexpr int kKmScanBlock = 1024;       // the one workgroup of k_kmeans_scan and k_kmeans_seed_pick
constexpr int kKmSeedRows = 64;          // rows per block sum of the seeding
constexpr int kKmSmallN = 64 * 512;      // below: tiles of 32 rows, twice as many workgroups
constexpr unsigned long long kKmNone = ~0ull;

__device__ __forceinline__ uint32_t km_key(float v) {   // ascending: lower first, -0.0 == +0.0, NaN after every number
    uint32_t bits = __float_as_uint(v);
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xfffffffeu;
    if (bits == 0x80000000u) bits = 0;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ float km_wave_sum(float s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

// sum (x_j - c_j)^2 over the row in float32: lanes stride the row, an fmaf chain per lane, xor butterfly.  nan: some x_j is a NaN
__device__ __forceinline__ float km_direct(const float* __restrict__ x, const float* __restrict__ c, int dim, int lane, bool* nan) {
    float s = 0.f;
    bool bad = false;
    for (int j = lane; j < dim; j += 64) {
        const float xv = x[j];
        bad |= xv != xv;
        const float d = xv - c[j];
        s = fmaf(d, d, s);
    }
    *nan = __ballot(bad) != 0ull;
    return km_wave_sum(s);
}

}  // namespace

// (stop: a device flag of kge_kmeans_run, set once no label moved -- the launches behind it return at once)
__global__ void __launch_bounds__(64) k_kmeans_begin(const int32_t* __restrict__ state, int* __restrict__ ctl) {
    if (threadIdx.x == 0) { ctl[0] = 0; ctl[1] = 0; ctl[2] = state[0]; ctl[3] = state[0]; }
}

__global__ void __launch_bounds__(kKmBlock) k_kmeans_cnorm(const float* __restrict__ cent, int k, int dim, int64_t cstride,
                                                            float* __restrict__ cnorm, const int* __restrict__ stop) {
    if (stop && *stop) return;
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * kKmWaves + (threadIdx.x >> 6);
    if (c >= k) return;
    const float* __restrict__ src = cent + (int64_t)c * cstride;
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) { const float v = src[i]; s = fmaf(v, v, s); }
    s = km_wave_sum(s);
    if (lane == 0) cnorm[c] = s;
}

template <int NQ>   // row tile of 32 * NQ
__global__ void __launch_bounds__(kKmBlock) k_kmeans_assign(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                             const float* __restrict__ cent, int k, int64_t cstride,
                                                             const float* __restrict__ cnorm, int32_t* __restrict__ label,
                                                             float* __restrict__ dist2, int* __restrict__ ctl, const int* __restrict__ stop) {
    constexpr int QT = 32 * NQ, QS = QT + 4, NLQ = QT / 8;
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    __shared__ float sC[kKmKS * kKmCS];
    __shared__ float sQ[kKmKS * QS];
    __shared__ float s_cn[kKmCT];
    __shared__ unsigned long long s_best[QT * 8];
    __shared__ int s_ctl[2];
    if (stop && *stop) return;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, lk = lane >> 5;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int ctiles = (k + kKmCT - 1) / kKmCT;
    const int nslab = (dim - 1) / kKmKS + 1;
    if (tid < 2) s_ctl[tid] = 0;

    // global -> registers -> LDS, one step ahead of the matrix cores: unconditional loads from addresses clamped into the tables,
    // what is a zero (past k, n or dim) is remembered in a bit mask and applied at the LDS store
    float rc[16], rq[NLQ];
    uint32_t ld_ok = 0;   // bit i: rc[i] is an element of the centroids, bit 16 + i: rq[i] of the rows
    int ld_t = 0, ld_s = 0;
    const int q_last = (int)((n - 1 - q0 < QT - 1) ? n - 1 - q0 : QT - 1);   // the tile's last row (n > q0: the grid covers n)
    auto load_step = [&]() __attribute__((always_inline)) {
        const int kd = ld_s * kKmKS + (tid & 31);
        const bool kin = kd < dim;
        const int kc = kin ? kd : dim - 1;
        ld_ok = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = ld_t * kKmCT + (tid >> 5) + 8 * i;
            const bool in = c < k;
            rc[i] = cent[(int64_t)(in ? c : k - 1) * cstride + kc];
            ld_ok |= (kin && in) ? 1u << i : 0u;
        }
#pragma unroll
        for (int i = 0; i < NLQ; ++i) {
            const int ql = (tid >> 5) + 8 * i;
            const bool in = ql <= q_last;
            rq[i] = rows[(q0 + (in ? ql : q_last)) * row_stride + kc];
            ld_ok |= (kin && in) ? 65536u << i : 0u;
        }
        if (++ld_s == nslab) { ld_s = 0; ++ld_t; }
    };

    f32x16 acc[NQ];
    unsigned long long best[NQ];
#pragma unroll
    for (int ni = 0; ni < NQ; ++ni) { acc[ni] = f32x16{0}; best[ni] = kKmNone; }
    load_step();
    __syncthreads();
    for (int ct = 0; ct < ctiles; ++ct) {
        float cn_mine = 0.f;
        if (tid < kKmCT) { const int c = ct * kKmCT + tid; cn_mine = cnorm[c < k ? c : k - 1]; }
        for (int sl = 0; sl < nslab; ++sl) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sC[(tid & 31) * kKmCS + (tid >> 5) + 8 * i] = (ld_ok >> i) & 1u ? rc[i] : 0.f;
#pragma unroll
            for (int i = 0; i < NLQ; ++i) sQ[(tid & 31) * QS + (tid >> 5) + 8 * i] = (ld_ok >> (16 + i)) & 1u ? rq[i] : 0.f;
            __syncthreads();
            if (ld_t < ctiles) load_step();
#pragma unroll
            for (int kk = 0; kk < kKmKS; kk += 2) {
                const float a = sC[(kk + lk) * kKmCS + wave * 32 + li];
#pragma unroll
                for (int ni = 0; ni < NQ; ++ni)
                    acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sQ[(kk + lk) * QS + ni * 32 + li], acc[ni], 0, 0, 0);
            }
            __syncthreads();   // the slab is consumed: the next fill may overwrite it
        }
        if (tid < kKmCT) s_cn[tid] = cn_mine;
        __syncthreads();
        // ---- the step's products are complete: the lane owns row (ni, li), register r is centroid cbase + (r & 3) + 8 (r >> 2).
        // The registers are not in ascending id order across lanes and waves: the compare is on the pair (key, id).
        const int cl = wave * 32 + 4 * lk;
        const int cbase = ct * kKmCT + cl;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = (r & 3) + 8 * (r >> 2);
            const int c = cbase + o;
            const float cn = s_cn[cl + o];
#pragma unroll
            for (int ni = 0; ni < NQ; ++ni) {
                const float key = cn - 2.0f * acc[ni][r];
                const unsigned long long p = ((unsigned long long)km_key(key) << 32) | (uint32_t)c;
                best[ni] = (c < k && p < best[ni]) ? p : best[ni];
            }
        }
#pragma unroll
        for (int ni = 0; ni < NQ; ++ni) acc[ni] = f32x16{0};
    }

    // ---- the eight partial winners of every row meet; one wave per row finishes it
#pragma unroll
    for (int ni = 0; ni < NQ; ++ni) s_best[(ni * 32 + li) * 8 + wave * 2 + lk] = best[ni];
    __syncthreads();
    for (int ql = wave; ql < QT; ql += kKmWaves) {
        const int64_t i = q0 + ql;
        if (i >= n) break;
        unsigned long long v = lane < 8 ? s_best[ql * 8 + lane] : kKmNone;
#pragma unroll
        for (int d = 4; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o < v ? o : v; }
        const int id = __builtin_amdgcn_readfirstlane((int)(uint32_t)v);   // < k: every row saw centroid 0
        bool nan;
        const float s = km_direct(rows + i * row_stride, cent + (int64_t)id * cstride, dim, lane, &nan);
        if (lane == 0) {
            const int32_t now = nan ? -1 : id;
            if (ctl) {
                if (label[i] != now) atomicAdd(&s_ctl[0], 1);
                if (nan) atomicAdd(&s_ctl[1], 1);
            }
            label[i] = now;
            dist2[i] = nan ? __uint_as_float(0x7fc00000u) : s;
        }
    }
    if (ctl) {
        __syncthreads();
        if (tid < 2 && s_ctl[tid]) atomicAdd(&ctl[tid], s_ctl[tid]);
    }
}

// block b ranks rows [1024 b, 1024 b + 1024): rank[i] = rows of the block before i with i's label; hist[b][c] = the block's rows of c
__global__ void __launch_bounds__(kKmBlock) k_kmeans_hist(const int32_t* __restrict__ label, int64_t n, int k, int32_t* __restrict__ rank,
                                                           int32_t* __restrict__ hist, const int* __restrict__ stop) {
    __shared__ int s_hist[KGE_KMEANS_MAX_K];
    __shared__ int s_lab[kKmBlock];
    if (stop && *stop) return;
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += kKmBlock) s_hist[c] = 0;
    for (int p = 0; p < kKmGroupRows / kKmBlock; ++p) {
        const int64_t i = (int64_t)blockIdx.x * kKmGroupRows + p * kKmBlock + tid;
        int lab = i < n ? label[i] : -1;
        lab = lab < k ? lab : -1;   // (a caller's label outside the clusters: in none)
        __syncthreads();
        s_lab[tid] = lab;
        __syncthreads();
        int before = 0, after = 0;
        if (lab >= 0) {
            for (int t = 0; t < kKmBlock; ++t) {
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
    for (int c = tid; c < k; c += kKmBlock) hist[(size_t)blockIdx.x * k + c] = s_hist[c];
}

// One workgroup.  hist[b][c] -> the rows of c in the blocks before b; off[c]: first place of cluster c in the member list; choff[c]:
// first chunk of cluster c (both [k + 1]).  With `state` (kge_kmeans_run): the inertia, the iteration's record and the stop flag
// of the NEXT iteration (this iteration's launches read the other one).
__global__ void __launch_bounds__(kKmScanBlock) k_kmeans_scan(int32_t* __restrict__ hist, int64_t nb, int k, int32_t* __restrict__ off,
                                                               int32_t* __restrict__ choff, const int32_t* __restrict__ label,
                                                               const float* __restrict__ dist2, int64_t n, double* __restrict__ inertia,
                                                               int32_t* __restrict__ state, int* __restrict__ ctl, int* __restrict__ stop_next,
                                                               const int* __restrict__ stop) {
    __shared__ int s_cnt[KGE_KMEANS_MAX_K];
    __shared__ int s_a[kKmScanBlock], s_b[kKmScanBlock];
    __shared__ double s_sum[kKmScanBlock];
    if (stop && *stop) {   // a stopped run stays stopped: the flag travels on to the iteration after this one
        if (threadIdx.x == 0) *stop_next = 1;
        return;
    }
    const int tid = threadIdx.x;
    for (int c = tid; c < k; c += kKmScanBlock) {
        int run = 0;
        for (int64_t b = 0; b < nb; ++b) { const int v = hist[b * k + c]; hist[b * k + c] = run; run += v; }
        s_cnt[c] = run;
    }
    __syncthreads();
    // exclusive scans over the clusters, four consecutive ones per thread (integers: any order gives the same sums)
    int mine = 0, mine_ch = 0;
    for (int j = 0; j < KGE_KMEANS_MAX_K / kKmScanBlock; ++j) {
        const int c = tid * (KGE_KMEANS_MAX_K / kKmScanBlock) + j;
        const int v = c < k ? s_cnt[c] : 0;
        mine += v;
        mine_ch += (v + KGE_KMEANS_CHUNK - 1) / KGE_KMEANS_CHUNK;
    }
    s_a[tid] = mine;
    s_b[tid] = mine_ch;
    __syncthreads();
    for (int d = 1; d < kKmScanBlock; d <<= 1) {
        const int a = tid >= d ? s_a[tid - d] : 0, b = tid >= d ? s_b[tid - d] : 0;
        __syncthreads();
        s_a[tid] += a;
        s_b[tid] += b;
        __syncthreads();
    }
    int run = s_a[tid] - mine, run_ch = s_b[tid] - mine_ch;
    for (int j = 0; j < KGE_KMEANS_MAX_K / kKmScanBlock; ++j) {
        const int c = tid * (KGE_KMEANS_MAX_K / kKmScanBlock) + j;
        if (c <= k) { off[c] = run; choff[c] = run_ch; }
        if (c < k) { run += s_cnt[c]; run_ch += (s_cnt[c] + KGE_KMEANS_CHUNK - 1) / KGE_KMEANS_CHUNK; }
    }
    if (tid == 0 && k == KGE_KMEANS_MAX_K) { off[k] = s_a[kKmScanBlock - 1]; choff[k] = s_b[kKmScanBlock - 1]; }
    if (!state) return;
    // the inertia: thread t adds rows t, t + 1024, ... in float64, then a tree over the threads -- a fixed order
    double s = 0.0;
    for (int64_t i = tid; i < n; i += kKmScanBlock) s += label[i] >= 0 ? (double)dist2[i] : 0.0;
    s_sum[tid] = s;
    __syncthreads();
    for (int d = kKmScanBlock / 2; d > 0; d >>= 1) {
        if (tid < d) s_sum[tid] += s_sum[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        const int changed = ctl[0];
        *inertia = s_sum[0];
        state[0] = changed == 0 ? 1 : 0;
        state[1] += 1;
        state[2] = changed;
        state[3] = ctl[1];
        *stop_next = changed == 0 ? 1 : 0;
        ctl[0] = 0;
        ctl[1] = 0;
    }
}

__global__ void __launch_bounds__(kKmBlock) k_kmeans_scatter(const int32_t* __restrict__ label, int64_t n, int k,
                                                              const int32_t* __restrict__ rank, const int32_t* __restrict__ hist,
                                                              const int32_t* __restrict__ off, int32_t* __restrict__ members,
                                                              const int* __restrict__ stop) {
    if (stop && *stop) return;
    const int64_t i = (int64_t)blockIdx.x * kKmBlock + threadIdx.x;
    if (i >= n) return;
    const int lab = label[i];
    if (lab >= 0 && lab < k) members[off[lab] + hist[(i / kKmGroupRows) * k + lab] + rank[i]] = (int32_t)i;
}

// wave = one chunk of one cluster, lane = one of 64 columns (blockIdx.y): the chunk's members added in member order in float32
__global__ void __launch_bounds__(kKmBlock) k_kmeans_update(const float* __restrict__ rows, int dim, int64_t row_stride, int k,
                                                             const int32_t* __restrict__ members, const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ choff, float* __restrict__ csum,
                                                             const int* __restrict__ stop) {
    if (stop && *stop) return;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kKmWaves + (threadIdx.x >> 6);
    if (g >= choff[k]) return;
    int lo = 0, hi = k;   // the last cluster c with choff[c] <= g (clusters without members share their successor's first chunk)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (choff[mid] <= g) lo = mid; else hi = mid; }
    const int c = lo;
    const int m0 = off[c] + (g - choff[c]) * KGE_KMEANS_CHUNK;
    const int m1 = (m0 + KGE_KMEANS_CHUNK < off[c + 1]) ? m0 + KGE_KMEANS_CHUNK : off[c + 1];
    for (int64_t c0 = (int64_t)blockIdx.y * 64; c0 < dim; c0 += (int64_t)gridDim.y * 64) {   // (the grid's y stops at 65 535 blocks)
        const int col = (int)c0 + lane;
        const int cc = col < dim ? col : dim - 1;
        float s = 0.f;
        for (int m = m0; m < m1; m += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = rows[(int64_t)members[m + j < m1 ? m + j : m1 - 1] * row_stride + cc];
#pragma unroll
            for (int j = 0; j < 8; ++j) s = m + j < m1 ? s + v[j] : s;
        }
        if (col < dim) csum[(size_t)g * dim + col] = s;
    }
}

__global__ void __launch_bounds__(kKmBlock) k_kmeans_finish(int dim, const int32_t* __restrict__ off, const int32_t* __restrict__ choff,
                                                             const float* __restrict__ csum, int unit, float* __restrict__ cent,
                                                             int64_t cstride, int32_t* __restrict__ count, const int* __restrict__ stop) {
    __shared__ double s_sq[kKmBlock];
    if (stop && *stop) return;
    const int tid = threadIdx.x, c = blockIdx.x;
    const int cnt = off[c + 1] - off[c], g0 = choff[c], g1 = choff[c + 1];
    if (cnt == 0) { if (tid == 0) count[c] = 0; return; }
    auto mean = [&](int col) {
        double s = 0.0;
        for (int g = g0; g < g1; ++g) s += (double)csum[(size_t)g * dim + col];
        return s / (double)cnt;
    };
    double inv = 1.0;
    if (unit) {
        double sq = 0.0;
        for (int col = tid; col < dim; col += kKmBlock) { const double m = mean(col); sq += m * m; }
        s_sq[tid] = sq;
        __syncthreads();
        for (int d = kKmBlock / 2; d > 0; d >>= 1) {
            if (tid < d) s_sq[tid] += s_sq[tid + d];
            __syncthreads();
        }
        const double norm = sqrt(s_sq[0]);
        if (!(norm > 0.0)) { if (tid == 0) count[c] = 0; return; }   // a mean without direction: the centroid stays
        inv = norm;
    }
    for (int col = tid; col < dim; col += kKmBlock) cent[(int64_t)c * cstride + col] = (float)(unit ? mean(col) / inv : mean(col));
    if (tid == 0) count[c] = cnt;
}

// d_i = min(d_i, |x_i - centre|^2) for the centre out_ids[j] (j == 0: d_i starts from +inf), 0 for a row with a NaN; bsum[b]: the
// float64 sum of block b's 64 rows in row order
__global__ void __launch_bounds__(kKmBlock) k_kmeans_seed_fold(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                                const int32_t* __restrict__ ids, int j, float* __restrict__ mind,
                                                                double* __restrict__ bsum) {
    __shared__ float s_d[kKmSeedRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ centre = rows + (int64_t)ids[j] * row_stride;
    for (int r = 0; r < kKmSeedRows / kKmWaves; ++r) {
        const int ql = wave * (kKmSeedRows / kKmWaves) + r;
        const int64_t i = (int64_t)blockIdx.x * kKmSeedRows + ql;
        float d = 0.f;
        if (i < n) {
            bool nan;
            const float s = km_direct(rows + i * row_stride, centre, dim, lane, &nan);
            const float old = j == 0 ? __uint_as_float(0x7f800000u) : mind[i];
            d = nan ? 0.f : (s < old ? s : old);
            if (lane == 0) mind[i] = d;
        }
        if (lane == 0) s_d[ql] = d;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int q = 0; q < kKmSeedRows; ++q) s += (double)s_d[q];
        bsum[blockIdx.x] = s;
    }
}

// One workgroup.  Centre j: for j == 0 the first row without a NaN from row floor(u[0] n) on (cyclically); else the first row whose inclusive float64 prefix of d passes u[j] T -- block
// sums scanned in order, then the rows of the one block --; the lowest row id not chosen yet when T is not positive.
__global__ void __launch_bounds__(kKmScanBlock) k_kmeans_seed_pick(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                                    int j, const double* __restrict__ u, const float* __restrict__ mind,
                                                                    const double* __restrict__ bsum, int64_t nb, int32_t* __restrict__ ids,
                                                                    float* __restrict__ centroids) {
    __shared__ double s_part[kKmScanBlock], s_off[kKmScanBlock + 1];
    __shared__ int s_first, s_pick;
    const int tid = threadIdx.x;
    if (j == 0) {
        int64_t i0 = (int64_t)floor(u[0] * (double)n);
        i0 = i0 < 0 ? 0 : i0 > n - 1 ? n - 1 : i0;
        int64_t found = i0;   // (every row holds a NaN: the row itself)
        for (int64_t a = 0; a < n; ++a) {   // the first row without a NaN, cyclically from i0 on: the first try almost always
            const int64_t r = i0 + a < n ? i0 + a : i0 + a - n;
            bool bad = false;
            for (int col = tid; col < dim; col += kKmScanBlock) { const float v = rows[r * row_stride + col]; bad |= v != v; }
            if (!__syncthreads_or(bad)) { found = r; break; }
        }
        if (tid == 0) s_pick = (int)found;
    } else {
        const int64_t L = (nb + kKmScanBlock - 1) / kKmScanBlock;
        const int64_t b0 = tid * L, b1 = b0 + L < nb ? b0 + L : nb;
        double lp = 0.0;
        for (int64_t b = b0; b < b1; ++b) lp += bsum[b];
        s_part[tid] = lp;
        if (tid == 0) { s_first = INT_MAX; s_pick = INT_MAX; }
        __syncthreads();
        if (tid == 0) {
            double run = 0.0;
            for (int t = 0; t < kKmScanBlock; ++t) { s_off[t] = run; run += s_part[t]; }
            s_off[kKmScanBlock] = run;
        }
        __syncthreads();
        const double T = s_off[kKmScanBlock], target = u[j] * T;
        lp = 0.0;
        for (int64_t b = b0; b < b1; ++b) {
            lp += bsum[b];
            if (s_off[tid] + lp > target) { atomicMin(&s_first, (int)b); break; }
        }
        __syncthreads();
        const int fb = s_first;
        if (T > 0.0 && fb != INT_MAX) {
            if (tid == 0) {
                const int64_t t = fb / L;
                double before = 0.0, ws = 0.0;
                for (int64_t b = t * L; b < fb; ++b) before += bsum[b];
                int64_t i = (int64_t)fb * kKmSeedRows;
                const int64_t end = i + kKmSeedRows < n ? i + kKmSeedRows : n;
                for (; i < end - 1; ++i) {
                    ws += (double)mind[i];
                    if (s_off[t] + (before + ws) > target) break;
                }
                s_pick = (int)i;   // (the block's last row passes: its prefix is the block's)
            }
        } else {
            for (int cand = tid; cand <= j && cand < n; cand += kKmScanBlock) {
                bool taken = false;
                for (int q = 0; q < j; ++q) taken |= ids[q] == cand;
                if (!taken) atomicMin(&s_pick, cand);
            }
        }
    }
    __syncthreads();
    const int id = s_pick;
    if (tid == 0) ids[j] = id;
    for (int col = tid; col < dim; col += kKmScanBlock) centroids[(size_t)j * dim + col] = rows[(int64_t)id * row_stride + col];
}

namespace {

struct KmPlan {
    int64_t nb, maxchunks, nbs;
    size_t o_cnorm, o_ctl, o_rank, o_hist, o_off, o_choff, o_members, o_csum, o_mind, o_bsum, bytes;
};

KmPlan km_plan(int64_t n, int64_t dim, int32_t k) {
    KmPlan p;
    p.nb = (n + kKmGroupRows - 1) / kKmGroupRows;
    p.maxchunks = n / KGE_KMEANS_CHUNK + k;          // sum over clusters of ceil(count / CHUNK) stays below
    p.nbs = (n + kKmSeedRows - 1) / kKmSeedRows;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    p.o_cnorm = take((size_t)k * sizeof(float));
    p.o_ctl = take(4 * sizeof(int));
    p.o_rank = take((size_t)n * sizeof(int32_t));
    p.o_hist = take((size_t)p.nb * k * sizeof(int32_t));
    p.o_off = take((size_t)(k + 1) * sizeof(int32_t));
    p.o_choff = take((size_t)(k + 1) * sizeof(int32_t));
    p.o_members = take((size_t)n * sizeof(int32_t));
    p.o_csum = take((size_t)p.maxchunks * dim * sizeof(float));
    p.o_mind = take((size_t)n * sizeof(float));
    p.o_bsum = take((size_t)p.nbs * sizeof(double));
    p.bytes = o + 256;   // + 256: the pointer is aligned up
    return p;
}

const char* km_check(const char* who, int64_t n, int64_t dim, int64_t k) {
    static thread_local char msg[200];
    if (n < 1 || n > 0x7fffff00ll) { snprintf(msg, sizeof msg, "%s: n = %lld outside 1..2^31-257 (row ids are int32)", who, (long long)n); return msg; }
    if (dim < 1 || dim > 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: dim = %lld outside 1..2^31-1", who, (long long)dim); return msg; }
    const int64_t most = n < KGE_KMEANS_MAX_K ? n : KGE_KMEANS_MAX_K;
    if (k < 1 || k > most) {
        snprintf(msg, sizeof msg, "%s: k = %lld outside 1..min(n = %lld, KGE_KMEANS_MAX_K = %d)", who, (long long)k, (long long)n, KGE_KMEANS_MAX_K);
        return msg;
    }
    return nullptr;
}

// the arguments every entry point shares; 0 and the aligned workspace in *base when they pass
int km_enter(const char* who, int64_t n, int64_t dim, int64_t row_stride, int64_t k, int64_t centroid_stride, void* workspace,
             size_t workspace_bytes, KmPlan* p, char** base) {
    if (const char* bad = km_check(who, n, dim, k)) { set_error("%s", bad); return -1; }
    if (row_stride < dim) { set_error("%s: row_stride = %lld < dim = %lld", who, (long long)row_stride, (long long)dim); return -1; }
    if (centroid_stride < dim) { set_error("%s: centroid_stride = %lld < dim = %lld", who, (long long)centroid_stride, (long long)dim); return -1; }
    *p = km_plan(n, dim, (int32_t)k);
    if (!workspace || workspace_bytes < p->bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_kmeans_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p->bytes);
        return -1;
    }
    *base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    return 0;
}

int km_assign(const KmPlan& p, char* base, const float* rows, int64_t n, int dim, int64_t row_stride, const float* cent, int k,
              int64_t cstride, int32_t* label, float* dist2, int* ctl, const int* stop, hipStream_t s) {
    float* cnorm = (float*)(base + p.o_cnorm);
    hipLaunchKernelGGL(k_kmeans_cnorm, dim3((unsigned)((k + kKmWaves - 1) / kKmWaves)), dim3(kKmBlock), 0, s, cent, k, dim, cstride, cnorm, stop);
    if (int rc = check_launch("k_kmeans_cnorm")) return rc;
    if (n >= kKmSmallN)
        hipLaunchKernelGGL((k_kmeans_assign<2>), dim3((unsigned)((n + 63) / 64)), dim3(kKmBlock), 0, s, rows, n, dim, row_stride, cent, k,
                           cstride, (const float*)cnorm, label, dist2, ctl, stop);
    else
        hipLaunchKernelGGL((k_kmeans_assign<1>), dim3((unsigned)((n + 31) / 32)), dim3(kKmBlock), 0, s, rows, n, dim, row_stride, cent, k,
                           cstride, (const float*)cnorm, label, dist2, ctl, stop);
    return check_launch("k_kmeans_assign");
}

int km_update(const KmPlan& p, char* base, const float* rows, int64_t n, int dim, int64_t row_stride, const int32_t* label, int k,
              int unit, float* cent, int64_t cstride, int32_t* count, const float* dist2, double* inertia, int32_t* state, int* ctl,
              int* stop_next, const int* stop, hipStream_t s) {
    int32_t* rank = (int32_t*)(base + p.o_rank);
    int32_t* hist = (int32_t*)(base + p.o_hist);
    int32_t* off = (int32_t*)(base + p.o_off);
    int32_t* choff = (int32_t*)(base + p.o_choff);
    int32_t* members = (int32_t*)(base + p.o_members);
    float* csum = (float*)(base + p.o_csum);
    hipLaunchKernelGGL(k_kmeans_hist, dim3((unsigned)p.nb), dim3(kKmBlock), 0, s, label, n, k, rank, hist, stop);
    if (int rc = check_launch("k_kmeans_hist")) return rc;
    hipLaunchKernelGGL(k_kmeans_scan, dim3(1), dim3(kKmScanBlock), 0, s, hist, p.nb, k, off, choff, label, dist2, n, inertia, state, ctl,
                       stop_next, stop);
    if (int rc = check_launch("k_kmeans_scan")) return rc;
    hipLaunchKernelGGL(k_kmeans_scatter, dim3((unsigned)((n + kKmBlock - 1) / kKmBlock)), dim3(kKmBlock), 0, s, label, n, k,
                       (const int32_t*)rank, (const int32_t*)hist, (const int32_t*)off, members, stop);
    if (int rc = check_launch("k_kmeans_scatter")) return rc;
    hipLaunchKernelGGL(k_kmeans_update, dim3((unsigned)((p.maxchunks + kKmWaves - 1) / kKmWaves), (unsigned)((dim + 63) / 64 < 65535 ? (dim + 63) / 64 : 65535)), dim3(kKmBlock),
                       0, s, rows, dim, row_stride, k, (const int32_t*)members, (const int32_t*)off, (const int32_t*)choff, csum, stop);
    if (int rc = check_launch("k_kmeans_update")) return rc;
    hipLaunchKernelGGL(k_kmeans_finish, dim3((unsigned)k), dim3(kKmBlock), 0, s, dim, (const int32_t*)off, (const int32_t*)choff,
                       (const float*)csum, unit, cent, cstride, count, stop);
    return check_launch("k_kmeans_finish");
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_kmeans_workspace_bytes(int64_t n, int64_t dim, int32_t k) {
    if (km_check("kge_kmeans_workspace_bytes", n, dim, k)) return 0;
    return km_plan(n, dim, k).bytes;
}

int kge_kmeans_assign(const float* rows, int64_t n, int64_t dim, int64_t row_stride, const float* centroids, int32_t k,
                      int64_t centroid_stride, void* workspace, size_t workspace_bytes, int32_t* out_label, float* out_dist2,
                      void* stream) {
    const char* who = "kge_kmeans_assign";
    KmPlan p;
    char* base;
    if (int rc = km_enter(who, n, dim, row_stride, k, centroid_stride, workspace, workspace_bytes, &p, &base)) return rc;
    if (!rows || !centroids || !out_label || !out_dist2) { set_error("%s: null rows / centroids / out_label / out_dist2", who); return -1; }
    return km_assign(p, base, rows, n, (int)dim, row_stride, centroids, k, centroid_stride, out_label, out_dist2, nullptr, nullptr,
                     (hipStream_t)stream);
}

int kge_kmeans_update(const float* rows, int64_t n, int64_t dim, int64_t row_stride, const int32_t* label, int32_t k,
                      int32_t unit_centroids, float* centroids, int64_t centroid_stride, int32_t* out_count, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const char* who = "kge_kmeans_update";
    KmPlan p;
    char* base;
    if (int rc = km_enter(who, n, dim, row_stride, k, centroid_stride, workspace, workspace_bytes, &p, &base)) return rc;
    if (!rows || !label || !centroids || !out_count) { set_error("%s: null rows / label / centroids / out_count", who); return -1; }
    return km_update(p, base, rows, n, (int)dim, row_stride, label, k, unit_centroids ? 1 : 0, centroids, centroid_stride, out_count,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int kge_kmeans_run(const float* rows, int64_t n, int64_t dim, int64_t row_stride, float* centroids, int32_t k, int64_t centroid_stride,
                   int32_t unit_centroids, int32_t max_iter, int32_t* label, float* out_dist2, int32_t* out_count, double* out_inertia,
                   int32_t* state, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_kmeans_run";
    KmPlan p;
    char* base;
    if (max_iter < 0) { set_error("%s: max_iter = %d is negative", who, (int)max_iter); return -1; }
    if (int rc = km_enter(who, n, dim, row_stride, k, centroid_stride, workspace, workspace_bytes, &p, &base)) return rc;
    if (!rows || !centroids || !label || !out_dist2 || !out_count || !out_inertia || !state) {
        set_error("%s: null rows / centroids / label / out_dist2 / out_count / out_inertia / state", who);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    int* ctl = (int*)(base + p.o_ctl);   // [0] labels changed, [1] invalid rows, [2 + (it & 1)] the stop flag iteration `it` reads
    hipLaunchKernelGGL(k_kmeans_begin, dim3(1), dim3(64), 0, s, (const int32_t*)state, ctl);
    if (int rc = check_launch("k_kmeans_begin")) return rc;
    for (int it = 0; it < max_iter; ++it) {
        const int* stop = ctl + 2 + (it & 1);
        if (int rc = km_assign(p, base, rows, n, (int)dim, row_stride, centroids, k, centroid_stride, label, out_dist2, ctl, stop, s)) return rc;
        if (int rc = km_update(p, base, rows, n, (int)dim, row_stride, label, k, unit_centroids ? 1 : 0, centroids, centroid_stride, out_count,
                               out_dist2, out_inertia, state, ctl, ctl + 2 + ((it + 1) & 1), stop, s))
            return rc;
    }
    return 0;
}

int kge_kmeans_seed(const float* rows, int64_t n, int64_t dim, int64_t row_stride, int32_t k, const double* u, void* workspace,
                    size_t workspace_bytes, int32_t* out_ids, float* out_centroids, void* stream) {
    const char* who = "kge_kmeans_seed";
    KmPlan p;
    char* base;
    if (int rc = km_enter(who, n, dim, row_stride, k, dim, workspace, workspace_bytes, &p, &base)) return rc;
    if (!rows || !u || !out_ids || !out_centroids) { set_error("%s: null rows / u / out_ids / out_centroids", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    float* mind = (float*)(base + p.o_mind);
    double* bsum = (double*)(base + p.o_bsum);
    for (int j = 0; j < k; ++j) {
        if (j > 0) {
            hipLaunchKernelGGL(k_kmeans_seed_fold, dim3((unsigned)p.nbs), dim3(kKmBlock), 0, s, rows, n, (int)dim, row_stride,
                               (const int32_t*)out_ids, j - 1, mind, bsum);
            if (int rc = check_launch("k_kmeans_seed_fold")) return rc;
        }
        hipLaunchKernelGGL(k_kmeans_seed_pick, dim3(1), dim3(kKmScanBlock), 0, s, rows, n, (int)dim, row_stride, j, u, (const float*)mind,
                           (const double*)bsum, p.nbs, out_ids, out_centroids);
        if (int rc = check_launch("k_kmeans_seed_pick")) return rc;
    }
    return 0;
}

}  // extern "C"
