// kge_dbscan.hip -- DBSCAN (Ester et al. 1996) of embedding rows: density clusters without a cluster count, rows in sparse regions
// labelled -1.  Three all-pairs passes on the matrix cores, no [n, n] block of any kind, no float atomics; every output is an integer
// and a unique function of the eps-graph, so nothing depends on the order in which work happens.
//
//   k_dbs_rows          one wave per row: |x|^2 in float32 (lanes stride the row, xor butterfly) and the row's state: bad for a row with
//                       a NaN entry -- nobody's neighbour, not even its own.
//   k_dbs_sweep         the one sweep of all three passes.  A workgroup of 4 waves owns 128 row slots and one slab of column tiles; each
//                       wave keeps 32 rows as the B operand of mfma_f32_32x32x2f32 for the whole sweep.  A step is 4 column tiles (128
//                       slots) gathered into k-major LDS slabs of 32 dims that the waves share, one fill ahead in registers (the fill
//                       machinery of k_sil_sweep).  After the last dim slab a lane holds 16 products of ONE row per tile, lane ^ 32 the
//                       other 16; the pair test max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 0) <= eps2 (cosine: max(1 - x_i.x_j, 0) <= eps) is
//                       made in registers and no distance leaves the wave.  The test is symmetric: the products of a pair meet in the
//                       same k order on either operand side, and the two norms are added to each other first.
//                         COUNT   rows: all, columns: all but the bad -> the hits of a row in the slab, an integer, to part[slab][row].
//                         ROUND   rows and columns: the ordered core list -> the least component id among the row's core neighbours
//                                 (read from the step's column records) is hooked by integer atomicMin onto the row's root and the row.
//                         BORDER  rows: the plain (neither core nor bad) ones, columns: the core list -> the least component id among
//                                 the core neighbours, atomicMin into rowmin[row].
//   k_dbs_core          one thread per row folds the slab partials into out_count, out_core and the row's state.
//   k_dbs_compact       one workgroup: the core rows in ascending id (ordered ranks: a chunk per thread, one scan), every core its own
//                       component; the number of cores stays on the device.
//   k_dbs_compress      pointer jumping: every core follows its chain to the root.  Also clears the change flag of the next round.
//   k_dbs_number        one workgroup: roots, in ascending id, are numbered 0, 1, ... (the same ordered ranks).
//   k_dbs_label         one thread per row: a core takes its root's number, a plain row that of rowmin (none: -1), a bad row -1.
//
// Component ids are positions in the ordered core list, so the least position is the least row id.  Invariants of the rounds: comp[p]
// <= p, and comp[p] is a core of p's component; integer min keeps both whatever a sweep reads while the same round writes.  A round that
// hooks nothing read a stable, fully compressed state in which no core has a neighbour of lower id: comp is then constant on every
// component and equal to its lowest core.  After round t every core is at or below the least id within t hops, so the rounds number
// at most 1 + the largest hop distance from a component's lowest core: never more than max(1, cores).
#include <climits>
#include <cmath>
#include <cstdio>
#include "kge_internal.h"

namespace kge {

namespace {

constexpr int kDbsBlock = 256;
constexpr int kDbsWaves = kDbsBlock / 64;
constexpr int kDbsRT = 32 * kDbsWaves;     // row slots of a workgroup
constexpr int kDbsTile = 32;
constexpr int kDbsStepTiles = 4;
constexpr int kDbsCT = kDbsTile * kDbsStepTiles;   // column slots per step
constexpr int kDbsKS = 32;                 // dim slab of one LDS fill
constexpr int kDbsCS = kDbsCT + 4;         // k-major operand rows, padded
constexpr int kDbsQS = kDbsRT + 4;
constexpr int kDbsScanBlock = 1024;
constexpr int kDbsMaxSplit = 64;
constexpr int kDbsTargetGroups = 256;      // one workgroup on each of 256 compute units

constexpr int kDbsCount = 0, kDbsRound = 1, kDbsBorder = 2;   // the sweep's modes
constexpr uint8_t kDbsPlain = 0, kDbsCore = 1, kDbsBad = 2;   // a row's state
// meta[0]: the number of cores; meta[1], meta[2]: the change flags of odd and even rounds
constexpr int kDbsMeta = 4;

// Ordered ranks inside one workgroup of 1024 threads: thread t owns the chunk [t per, t per + per) of 0..total-1, counts its hits,
// one scan over the threads, then emit(i, hit, hits before i) in ascending i.  Returns the number of hits.
template <class P, class E>
__device__ __forceinline__ int dbs_ordered_ranks(int64_t total, int* s_a, P pred, E emit) {
    const int tid = threadIdx.x;
    const int64_t per = (total + kDbsScanBlock - 1) / kDbsScanBlock;
    const int64_t lo = tid * per < total ? tid * per : total, hi = lo + per < total ? lo + per : total;
    int mine = 0;
    for (int64_t i = lo; i < hi; ++i) mine += pred(i) ? 1 : 0;
    s_a[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kDbsScanBlock; d <<= 1) {
        const int a = tid >= d ? s_a[tid - d] : 0;
        __syncthreads();
        s_a[tid] += a;
        __syncthreads();
    }
    int run = s_a[tid] - mine;
    for (int64_t i = lo; i < hi; ++i) { const bool hit = pred(i); emit(i, hit, run); run += hit ? 1 : 0; }
    return s_a[kDbsScanBlock - 1];
}

}  // namespace

__global__ void __launch_bounds__(kDbsBlock) k_dbs_rows(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride,
                                                         float* __restrict__ norm, uint8_t* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kDbsWaves + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* __restrict__ src = rows + i * row_stride;
    float s = 0.f;
    bool bad = false;
    for (int j = lane; j < dim; j += 64) { const float v = src[j]; bad |= v != v; s = fmaf(v, v, s); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    const bool nan = __ballot(bad) != 0ull;
    if (lane == 0) { norm[i] = s; state[i] = nan ? kDbsBad : kDbsPlain; }
}

template <int MODE, bool COS>
__global__ void __launch_bounds__(kDbsBlock) k_dbs_sweep(const float* __restrict__ rows, int64_t n, int dim, int64_t row_stride, float thr,
                                                          const float* __restrict__ norm, const uint8_t* __restrict__ state,
                                                          const int32_t* __restrict__ list, const int32_t* __restrict__ meta,
                                                          int32_t* comp /* read while the round writes it */,
                                                          int32_t* __restrict__ out /* COUNT: part [S][n]; BORDER: rowmin [n] */,
                                                          int32_t* __restrict__ changed) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    __shared__ float sC[kDbsKS * kDbsCS];
    __shared__ float sQ[kDbsKS * kDbsQS];
    __shared__ int4 s_col[2][kDbsCT];   // (key or -1, the bits of |x|^2, the component id) of the step's slots, by step parity

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, lk = lane >> 5;
    const int n_rows = (int)n;   // (row ids are int32)
    const int cores = MODE == kDbsCount ? 0 : meta[0];
    const int nr = MODE == kDbsRound ? cores : n_rows, nc = MODE == kDbsCount ? n_rows : cores;
    const int q0 = blockIdx.x * kDbsRT;
    if (q0 >= nr) return;   // (the grid covers n row slots; the core list may be shorter)
    const int T = (nc + kDbsTile - 1) / kDbsTile;
    const int t0 = (int)((int64_t)T * blockIdx.y / gridDim.y), t1 = (int)((int64_t)T * (blockIdx.y + 1) / gridDim.y);
    const int lim = t1 * kDbsTile < nc ? t1 * kDbsTile : nc;   // the slab's column slots end here
    const int steps = (t1 - t0 + kDbsStepTiles - 1) / kDbsStepTiles;
    const int nslab = (dim - 1) / kDbsKS + 1;
    const int q_last = (nr - 1 - q0 < kDbsRT - 1) ? nr - 1 - q0 : kDbsRT - 1;
    const int my_slot = q0 + wave * 32 + li;
    const int my_sc = my_slot < nr ? my_slot : nr - 1;
    const int my_row = MODE == kDbsRound ? list[my_sc] : my_sc;
    const int my_key = MODE == kDbsRound ? my_slot : my_row;   // what a column's key is compared with: a row is its own neighbour by index
    const float xn = norm[my_row];
    const uint8_t my_state = state[my_row];
    const bool active = my_slot < nr && (MODE == kDbsCount ? my_state != kDbsBad : MODE == kDbsRound ? true : my_state == kDbsPlain);
    if (MODE == kDbsBorder && !__syncthreads_or(active ? 1 : 0)) return;   // every row of the workgroup is a core or bad

    // global -> registers -> LDS, one fill ahead of the matrix cores: unconditional loads from addresses clamped into the tables, what
    // is a zero (a bad column, past the slab or dim) is remembered in a bit mask and applied at the LDS store
    float rc[16], rq[16];
    const float* cp[16];
    const float* qp[16];
    int4 col_rec = make_int4(-1, 0, INT_MAX, 0);
    uint32_t row_ok = 0, ld_ok = 0;   // bit i: cp[i] is a live column, bit 16 + i: qp[i] is a row slot below nr; ld_ok: those inside dim
    int ld_t = 0, ld_s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ql = (tid >> 5) + 8 * i;
        const bool in = ql <= q_last;
        const int slot = q0 + (in ? ql : q_last);
        qp[i] = rows + (int64_t)(MODE == kDbsRound ? list[slot] : slot) * row_stride;
        asm volatile("" : "+v"(qp[i]));
        row_ok |= in ? 65536u << i : 0u;
    }
    auto load_step = [&]() __attribute__((always_inline)) {
        if (ld_s == 0) {   // a new step: its columns
            const int base = (t0 + ld_t * kDbsStepTiles) * kDbsTile;
            row_ok &= 0xffff0000u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = base + (tid >> 5) + 8 * i;
                const int jc = j < lim ? j : lim - 1;
                const int m = MODE == kDbsCount ? jc : list[jc];
                const bool in = j < lim && (MODE != kDbsCount || state[m] != kDbsBad);
                cp[i] = rows + (int64_t)m * row_stride;
                asm volatile("" : "+v"(cp[i]));
                row_ok |= in ? 1u << i : 0u;
            }
            if (tid < kDbsCT) {
                const int j = base + tid;
                const int jc = j < lim ? j : lim - 1;
                const int m = MODE == kDbsCount ? jc : list[jc];
                const bool in = j < lim && (MODE != kDbsCount || state[m] != kDbsBad);
                col_rec.x = in ? (MODE == kDbsRound ? j : m) : -1;
                col_rec.y = (int)__float_as_uint(norm[m]);
                col_rec.z = MODE == kDbsCount ? 0 : comp[jc];
            }
        }
        const int kd = ld_s * kDbsKS + (tid & 31);
        const bool kin = kd < dim;
        const int kc = kin ? kd : dim - 1;
        ld_ok = kin ? row_ok : 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) rc[i] = cp[i][kc];
#pragma unroll
        for (int i = 0; i < 16; ++i) rq[i] = qp[i][kc];
        if (++ld_s == nslab) { ld_s = 0; ++ld_t; }
    };

    int found = MODE == kDbsCount ? 0 : INT_MAX;   // the row's hits, or the least component id among them: identical in both lane halves
    f32x16 acc[kDbsStepTiles];
#pragma unroll
    for (int ct = 0; ct < kDbsStepTiles; ++ct) acc[ct] = f32x16{0};
    if (steps > 0) load_step();
    for (int st = 0; st < steps; ++st) {
        for (int sl = 0; sl < nslab; ++sl) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sC[(tid & 31) * kDbsCS + (tid >> 5) + 8 * i] = (ld_ok >> i) & 1u ? rc[i] : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sQ[(tid & 31) * kDbsQS + (tid >> 5) + 8 * i] = (ld_ok >> (16 + i)) & 1u ? rq[i] : 0.f;
            if (sl == 0 && tid < kDbsCT) s_col[st & 1][tid] = col_rec;
            __syncthreads();
            if (ld_t < steps) load_step();
#pragma unroll
            for (int kk = 0; kk < kDbsKS; kk += 2) {
                const float b = sQ[(kk + lk) * kDbsQS + wave * 32 + li];
#pragma unroll
                for (int ct = 0; ct < kDbsStepTiles; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(sC[(kk + lk) * kDbsCS + ct * 32 + li], b, acc[ct], 0, 0, 0);
            }
            __syncthreads();   // the slab is consumed: the next fill may overwrite it
        }
        // ---- the step's products are complete: the lane owns row li of its wave, register r of block ct is slot
        // ct * 32 + (r & 3) + 8 (r >> 2) + 4 lk of the step
#pragma unroll
        for (int ct = 0; ct < kDbsStepTiles; ++ct) {
            if (t0 + st * kDbsStepTiles + ct < t1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int4 col = s_col[st & 1][ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk];
                    float d;
                    if (COS) d = fmaxf(1.0f - acc[ct][r], 0.f);
                    else d = fmaxf((xn + __uint_as_float((uint32_t)col.y)) - 2.0f * acc[ct][r], 0.f);
                    const bool hit = col.x >= 0 && (col.x == my_key || d <= thr);
                    if (MODE == kDbsCount) found += hit ? 1 : 0;
                    else found = hit && col.z < found ? col.z : found;
                }
            }
            acc[ct] = f32x16{0};
        }
    }
    const int other = __shfl_xor(found, 32);
    if (MODE == kDbsCount) {
        if (lk == 0 && my_slot < nr) out[(size_t)blockIdx.y * (size_t)n + (size_t)my_slot] = active ? found + other : 0;
    } else {
        const int least = other < found ? other : found;
        if (lk == 0 && active && least != INT_MAX) {
            if (MODE == kDbsBorder) atomicMin(&out[my_row], least);
            else {
                const int root = comp[my_slot];
                if (least < root) { atomicMin(&comp[root], least); atomicMin(&comp[my_slot], least); *changed = 1; }
            }
        }
    }
}

__global__ void __launch_bounds__(kDbsBlock) k_dbs_core(int64_t n, int S, int min_samples, const int32_t* __restrict__ part,
                                                         uint8_t* __restrict__ state, int32_t* __restrict__ out_count,
                                                         uint8_t* __restrict__ out_core, int32_t* __restrict__ rowmin) {
    const int64_t i = (int64_t)blockIdx.x * kDbsBlock + threadIdx.x;
    if (i >= n) return;
    int count = 0;
    for (int s = 0; s < S; ++s) count += part[(size_t)s * (size_t)n + (size_t)i];
    const bool core = state[i] != kDbsBad && count >= min_samples;
    out_count[i] = count;
    out_core[i] = core ? 1 : 0;
    if (core) state[i] = kDbsCore;
    rowmin[i] = INT_MAX;
}

__global__ void __launch_bounds__(kDbsScanBlock) k_dbs_compact(int64_t n, const uint8_t* __restrict__ state, int32_t* __restrict__ list,
                                                                int32_t* __restrict__ pos, int32_t* __restrict__ comp,
                                                                int32_t* __restrict__ meta) {
    __shared__ int s_a[kDbsScanBlock];
    const int cores = dbs_ordered_ranks(n, s_a, [&](int64_t i) { return state[i] == kDbsCore; },
                                        [&](int64_t i, bool hit, int before) {
                                            pos[i] = hit ? before : -1;
                                            if (hit) { list[before] = (int32_t)i; comp[before] = before; }
                                        });
    if (threadIdx.x == 0) { meta[0] = cores; meta[1] = 0; meta[2] = 0; }
}

__global__ void __launch_bounds__(kDbsBlock) k_dbs_compress(const int32_t* __restrict__ meta, int32_t* comp, int32_t* __restrict__ clear) {
    const int p = blockIdx.x * kDbsBlock + threadIdx.x;
    if (p == 0) *clear = 0;
    if (p >= meta[0]) return;
    int c = comp[p];
    for (int up = comp[c]; up < c; up = comp[c]) c = up;   // ids fall strictly along a chain: it ends at a root
    comp[p] = c;
}

__global__ void __launch_bounds__(kDbsScanBlock) k_dbs_number(const int32_t* __restrict__ meta, const int32_t* __restrict__ comp,
                                                               int32_t* __restrict__ number, int32_t* __restrict__ out_n_clusters) {
    __shared__ int s_a[kDbsScanBlock];
    const int roots = dbs_ordered_ranks(meta[0], s_a, [&](int64_t p) { return comp[p] == (int32_t)p; },
                                        [&](int64_t p, bool hit, int before) { if (hit) number[p] = before; });
    if (threadIdx.x == 0) out_n_clusters[0] = roots;
}

__global__ void __launch_bounds__(kDbsBlock) k_dbs_label(int64_t n, const uint8_t* __restrict__ state, const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ comp, const int32_t* __restrict__ number,
                                                          const int32_t* __restrict__ rowmin, int rounds, int32_t* __restrict__ out_label,
                                                          int32_t* __restrict__ out_rounds) {
    const int64_t i = (int64_t)blockIdx.x * kDbsBlock + threadIdx.x;
    if (i == 0) out_rounds[0] = rounds;
    if (i >= n) return;
    const uint8_t st = state[i];
    int label = -1;
    if (st == kDbsCore) label = number[comp[pos[i]]];
    else if (st == kDbsPlain && rowmin[i] != INT_MAX) label = number[rowmin[i]];   // (rowmin holds roots: the last round compressed)
    out_label[i] = label;
}

namespace {

struct DbsPlan {
    int64_t rtiles;
    int S;
    size_t o_norm, o_state, o_part, o_list, o_pos, o_comp, o_number, o_rowmin, o_meta, bytes;
};

// The column split is a function of n alone: enough slabs that the row tiles fill the device; KGE_DBS_SPLIT forces it
DbsPlan dbs_plan(int64_t n) {
    DbsPlan p;
    p.rtiles = (n + kDbsRT - 1) / kDbsRT;
    int64_t want = switch_value("DBS_SPLIT");
    if (want < 1) want = kDbsTargetGroups / p.rtiles;
    if (want > kDbsMaxSplit) want = kDbsMaxSplit;
    if (want < 1) want = 1;
    p.S = (int)want;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    p.o_norm = take((size_t)n * sizeof(float));
    p.o_state = take((size_t)n);
    p.o_part = take((size_t)p.S * n * sizeof(int32_t));
    p.o_list = take((size_t)n * sizeof(int32_t));
    p.o_pos = take((size_t)n * sizeof(int32_t));
    p.o_comp = take((size_t)n * sizeof(int32_t));
    p.o_number = take((size_t)n * sizeof(int32_t));
    p.o_rowmin = take((size_t)n * sizeof(int32_t));
    p.o_meta = take((size_t)kDbsMeta * sizeof(int32_t));
    p.bytes = o + 256;   // + 256: the pointer is aligned up
    return p;
}

const char* dbs_check(const char* who, int64_t n, int64_t dim) {
    static thread_local char msg[200];
    if (n < 1 || n > 0x7ffe0000ll) { snprintf(msg, sizeof msg, "%s: n = %lld outside 1..2^31-2^17 (row ids are int32)", who, (long long)n); return msg; }
    if (dim < 1 || dim > 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: dim = %lld outside 1..2^31-1", who, (long long)dim); return msg; }
    return nullptr;
}

template <int MODE>
void dbs_sweep(bool cosine, dim3 grid, hipStream_t s, const float* rows, int64_t n, int dim, int64_t row_stride, float thr, const float* norm,
               const uint8_t* state, const int32_t* list, const int32_t* meta, int32_t* comp, int32_t* out, int32_t* changed) {
    if (cosine)
        hipLaunchKernelGGL((k_dbs_sweep<MODE, true>), grid, dim3(kDbsBlock), 0, s, rows, n, dim, row_stride, thr, norm, state, list, meta, comp,
                           out, changed);
    else
        hipLaunchKernelGGL((k_dbs_sweep<MODE, false>), grid, dim3(kDbsBlock), 0, s, rows, n, dim, row_stride, thr, norm, state, list, meta, comp,
                           out, changed);
}

}  // namespace

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_dbscan_workspace_bytes(int64_t n, int64_t dim) {
    if (dbs_check("kge_dbscan_workspace_bytes", n, dim)) return 0;
    return dbs_plan(n).bytes;
}

int kge_dbscan(const float* rows, int64_t n, int64_t dim, int64_t row_stride, float eps, int32_t min_samples, int metric,
               void* workspace, size_t workspace_bytes, int32_t* out_label, uint8_t* out_core, int32_t* out_count,
               int32_t* out_n_clusters, int32_t* out_rounds, void* stream) {
    const char* who = "kge_dbscan";
    if (const char* bad = dbs_check(who, n, dim)) { set_error("%s", bad); return -1; }
    if (row_stride < dim) { set_error("%s: row_stride = %lld < dim = %lld", who, (long long)row_stride, (long long)dim); return -1; }
    if (!std::isfinite(eps) || eps < 0.f) { set_error("%s: eps = %g is not a finite distance >= 0", who, (double)eps); return -1; }
    if (min_samples < 1) { set_error("%s: min_samples = %d below 1", who, (int)min_samples); return -1; }
    if (metric != KGE_DBS_L2 && metric != KGE_DBS_COSINE) { set_error("%s: metric = %d (0 = l2, 1 = cosine)", who, metric); return -1; }
    if (!rows || !out_label || !out_core || !out_count || !out_n_clusters || !out_rounds) {
        set_error("%s: null rows / out_label / out_core / out_count / out_n_clusters / out_rounds", who);
        return -1;
    }
    const DbsPlan p = dbs_plan(n);
    if (!workspace || workspace_bytes < p.bytes) {
        set_error("%s: workspace too small (%zu bytes, kge_dbscan_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, p.bytes);
        return -1;
    }
    char* base = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* norm = (float*)(base + p.o_norm);
    uint8_t* state = (uint8_t*)(base + p.o_state);
    int32_t* part = (int32_t*)(base + p.o_part);
    int32_t* list = (int32_t*)(base + p.o_list);
    int32_t* pos = (int32_t*)(base + p.o_pos);
    int32_t* comp = (int32_t*)(base + p.o_comp);
    int32_t* number = (int32_t*)(base + p.o_number);
    int32_t* rowmin = (int32_t*)(base + p.o_rowmin);
    int32_t* meta = (int32_t*)(base + p.o_meta);
    hipStream_t s = (hipStream_t)stream;
    const bool cosine = metric == KGE_DBS_COSINE;
    // eps^2 is formed in float64 and rounded to float32 once
    const float thr = cosine ? eps : (float)((double)eps * (double)eps);
    const unsigned row_blocks = (unsigned)((n + kDbsBlock - 1) / kDbsBlock);
    const dim3 grid((unsigned)p.rtiles, (unsigned)p.S);

    hipLaunchKernelGGL(k_dbs_rows, dim3((unsigned)((n + kDbsWaves - 1) / kDbsWaves)), dim3(kDbsBlock), 0, s, rows, n, (int)dim, row_stride, norm,
                       state);
    if (int rc = check_launch("k_dbs_rows")) return rc;
    dbs_sweep<kDbsCount>(cosine, grid, s, rows, n, (int)dim, row_stride, thr, norm, state, list, meta, comp, part, nullptr);
    if (int rc = check_launch("k_dbs_sweep (counts)")) return rc;
    hipLaunchKernelGGL(k_dbs_core, dim3(row_blocks), dim3(kDbsBlock), 0, s, n, p.S, (int)min_samples, (const int32_t*)part, state, out_count,
                       out_core, rowmin);
    if (int rc = check_launch("k_dbs_core")) return rc;
    hipLaunchKernelGGL(k_dbs_compact, dim3(1), dim3(kDbsScanBlock), 0, s, n, (const uint8_t*)state, list, pos, comp, meta);
    if (int rc = check_launch("k_dbs_compact")) return rc;

    // the labelling rounds: the host reads the round's change flag, one int32, and stops after the round that changed nothing
    int rounds = 0;
    for (;;) {
        ++rounds;
        int32_t* flag = meta + 1 + (rounds & 1);
        dbs_sweep<kDbsRound>(cosine, grid, s, rows, n, (int)dim, row_stride, thr, norm, state, list, meta, comp, nullptr, flag);
        if (int rc = check_launch("k_dbs_sweep (round)")) return rc;
        hipLaunchKernelGGL(k_dbs_compress, dim3(row_blocks), dim3(kDbsBlock), 0, s, (const int32_t*)meta, comp, meta + 1 + ((rounds + 1) & 1));
        if (int rc = check_launch("k_dbs_compress")) return rc;
        int32_t changed = 0;
        if (hipMemcpyAsync(&changed, flag, sizeof(changed), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            set_error("%s: reading the change flag of round %d failed", who, rounds);
            return -2;
        }
        if (!changed) break;
        if (rounds > n) { set_error("%s: %d labelling rounds over %lld rows: the bound is the number of cores", who, rounds, (long long)n); return -3; }
    }

    dbs_sweep<kDbsBorder>(cosine, grid, s, rows, n, (int)dim, row_stride, thr, norm, state, list, meta, comp, rowmin, nullptr);
    if (int rc = check_launch("k_dbs_sweep (border)")) return rc;
    hipLaunchKernelGGL(k_dbs_number, dim3(1), dim3(kDbsScanBlock), 0, s, (const int32_t*)meta, (const int32_t*)comp, number, out_n_clusters);
    if (int rc = check_launch("k_dbs_number")) return rc;
    hipLaunchKernelGGL(k_dbs_label, dim3(row_blocks), dim3(kDbsBlock), 0, s, n, (const uint8_t*)state, (const int32_t*)pos, (const int32_t*)comp,
                       (const int32_t*)number, (const int32_t*)rowmin, rounds, out_label, out_rounds);
    return check_launch("k_dbs_label");
}

}  // extern "C"
