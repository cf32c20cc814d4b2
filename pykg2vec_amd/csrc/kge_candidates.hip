// kge_candidates.hip -- ranking against GIVEN candidates: for query i, where does the true entity stand among the ids of list L(i)?
// The cost scales with the lists, not with the entity table (OGB-style fixed negatives, type-constrained ranking).
//
//   items    an item is (query, chunk of KGE_CAND_CHUNK consecutive entries of its list).  k_cand_items turns the list lengths into
//            the prefix sums item_off [n + 1] in the workspace (one workgroup, integer scan) and leaves a copy of the call's
//            arguments next to them; the ranking kernel grid-strides over item_off[n] items and finds an item's query by binary
//            search in item_off.  No host read anywhere.
//   kernel   k_rank_candidates<M, G, NCH>, the row kernels' geometry (kge_row_kernels.h): one G-lane group per item.  The group loads
//            the query's own rows (the roles whose id is NOT the swept column) once.  It then walks entries: first the true entity
//            alone, whose score it keeps as s_true, then per step of G list entries the live ones.  In such a step every lane
//            takes one entry and decides its liveness (range check -- an id outside [0, E) is never used as a row index --, not
//            the true id, binary search in the query's ascending skip segment: G searches in flight); a ballot gives the group the
//            mask of live entries, and the id travels with "left out by the filter" in its sign.  Per walked entry only the roles
//            whose id is the swept column (role_sel == 2 for tails, 0 for heads; SimplE's crossed roles included) are gathered,
//            and model_fwd runs on the same row values in the same geometry as k_score_fwd (-ffp-contract=off, no fast-math), so
//            the compared scores are kge_score_forward's bit for bit, whatever the compiler hoists out of the walk.
//   counts   four integer counters per group, added with integer atomicAdd to counts [4, n], which a memset on the stream zeroed:
//            the result does not depend on the arrival order.
//   scalars  the kernel is held to k_score_fwd's resources (no scratch or spill where that has none, tests/test_candidates_resources.py).
//            What overflowed at first were scalar registers, hence: rows are loaded without lane masks (load_row_nomask), the
//            arguments are read from the workspace copy, and ONE walk loop serves the true entity and the candidates, so that
//            model_fwd (RotatE: 2 * NCH sincosf chains) is instantiated once.
//   shared   with kge_relations.hip, in kge_rank_common.h: load_row_nomask, the list of row-kernel models, and the entry point's
//            opening (rank_entry_checks, rank_counts_begin); what is checked here is the lists' own.
// kge_rank_lists_from_scores is the counting half alone, for the models whose scores come from their own batch scorer: one wave
// per segment of scores, integer wave reductions, plain stores.
#include "kge_rank_common.h"

namespace kge {

namespace {

constexpr int kCandChunk = KGE_CAND_CHUNK;
constexpr int kItemsBlock = 1024;

struct CandArgs {
    const int64_t* triples; int64_t n; int side;
    const int64_t* list_of_query; const int64_t* cand_off; const int32_t* cand_ids; int64_t n_lists;
    const int64_t* skip_off; const int32_t* skip_ids;
    const int64_t* item_off; int64_t E; int32_t* counts;
};

// entries [lo, hi) of query q's list; an out-of-range list index is an empty list
__device__ __forceinline__ void cand_span(const CandArgs& a, int64_t q, int64_t& lo, int64_t& hi) {
    const int64_t l = a.list_of_query ? a.list_of_query[q] : q;
    lo = hi = 0;
    if (l >= 0 && l < a.n_lists) { lo = a.cand_off[l]; hi = a.cand_off[l + 1]; }
    if (hi < lo) hi = lo;
}

}  // namespace

// item_off[q] = number of items of the queries before q, item_off[n] = all items
__global__ void __launch_bounds__(kItemsBlock) k_cand_items(CandArgs a, int64_t* __restrict__ item_off, CandArgs* __restrict__ args_out) {
    __shared__ int64_t s_sum[kItemsBlock];
    const int tid = threadIdx.x;
    const int64_t per = (a.n + kItemsBlock - 1) / kItemsBlock;
    const int64_t q0 = min(a.n, tid * per), q1 = min(a.n, q0 + per);
    int64_t mine = 0;
    for (int64_t q = q0; q < q1; ++q) {
        int64_t lo, hi;
        cand_span(a, q, lo, hi);
        mine += (hi - lo + kCandChunk - 1) / kCandChunk;
    }
    s_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kItemsBlock; d <<= 1) {   // inclusive scan
        const int64_t up = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += up;
        __syncthreads();
    }
    int64_t run = s_sum[tid] - mine;
    for (int64_t q = q0; q < q1; ++q) {
        int64_t lo, hi;
        cand_span(a, q, lo, hi);
        item_off[q] = run;
        run += (hi - lo + kCandChunk - 1) / kCandChunk;
    }
    if (tid == kItemsBlock - 1) item_off[a.n] = s_sum[tid];
    if (tid == 0) {   // (field by field: a struct copy goes through a stack object that the compiler then parks in LDS)
        args_out->triples = a.triples; args_out->n = a.n; args_out->side = a.side;
        args_out->list_of_query = a.list_of_query; args_out->cand_off = a.cand_off; args_out->cand_ids = a.cand_ids;
        args_out->n_lists = a.n_lists; args_out->skip_off = a.skip_off; args_out->skip_ids = a.skip_ids;
        args_out->item_off = a.item_off; args_out->E = a.E; args_out->counts = a.counts;
    }
}

template <int M, int G, int NCH>
__global__ __launch_bounds__(kBlock) void k_rank_candidates(DeviceModel m, const CandArgs* args) {
    // (the arguments are read from the workspace copy where they are used -- a few scalar loads per item -- instead of occupying
    // two dozen scalar registers for the whole kernel: next to model_fwd's own scalars those no longer fit for RotatE / KG2E)
    const CandArgs& a = *args;
    constexpr int GPB = kBlock / G;
    constexpr int NR = role_count(M);
    const int gl = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) / G * G;   // first lane of the group inside its wave
    const int csel = a.side ? 0 : 2;                // the triple column the candidates replace
    const int n = (int)a.n;
    const int64_t n_items = a.item_off[n];
    for (int64_t it = (int64_t)blockIdx.x * GPB + threadIdx.x / G; it < n_items; it += (int64_t)gridDim.x * GPB) {
        // the query of this item: the last q with item_off[q] <= it
        int q = 0;
        for (int qh = n; qh - q > 1;) {
            const int mid = (int)(((unsigned)q + (unsigned)qh) >> 1);
            if (a.item_off[mid] <= it) q = mid; else qh = mid;
        }
        const int32_t* cand;   // this item's entries: cand[0 .. cnt)
        int cnt;
        {
            int64_t lo, hi;
            cand_span(a, q, lo, hi);
            lo += (it - a.item_off[q]) * kCandChunk;
            cnt = (int)min(hi - lo, (int64_t)kCandChunk);
            cand = a.cand_ids + lo;
        }
        int64_t id[3] = {a.triples[3 * (int64_t)q], a.triples[3 * (int64_t)q + 1], a.triples[3 * (int64_t)q + 2]};
        const int truth = (int)id[csel];
        const int32_t* skip = nullptr;   // the query's ascending skip segment: skip[0 .. n_skip)
        int n_skip = 0;
        if (a.skip_off) { skip = a.skip_ids + a.skip_off[q]; n_skip = (int)(a.skip_off[q + 1] - a.skip_off[q]); }
        Rows<M, NCH> R;   // the query's own rows now; the rows of the swept column come per walked entry
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (role_sel(M, r) != 1 && role_sel(M, r) == csel) continue;
            const int d = role_dim<M>(m, r);
            load_row_nomask<G, NCH>(R.x[r], m.tab[role_tab(M, r)] + id[role_sel(M, r)] * (int64_t)d, d, gl);
        }
        Saved<M, NCH> sv;
        float s_true = 0.f;
        int c_lt = 0, c_flt = 0, c_eq = 0, c_feq = 0;
        // step -G walks ONE entry, the true entity, and keeps its score; the steps from 0 on take G list entries each.  One walk
        // loop, so model_fwd is instantiated once per kernel (two copies of RotatE's sincosf chains run out of scalar registers).
        for (int base = -G; base < cnt; base += G) {
            const int j = base + gl;
            const bool first = base < 0;   // group-uniform
            const int e = first ? (gl == 0 ? truth : -1) : (j < cnt ? cand[j] : -1);
            const bool live = first ? gl == 0 : (e >= 0 && (int64_t)e < a.E && e != truth);
            bool kept = live;
            if (live && !first) {   // is e in the skip segment?
                int l = 0, h = n_skip;
                while (l < h) {
                    const int mid = (l + h) >> 1;
                    if (skip[mid] < e) l = mid + 1; else h = mid;
                }
                kept = !(l < n_skip && skip[l] == e);
            }
            const int mine = kept ? e : ~e;   // the id and, in its sign, "left out by the filter": one value to hand round
            unsigned long long m_live = __ballot(live) >> gbase;
            if constexpr (G < 64) m_live &= (1ull << G) - 1ull;
            while (m_live) {   // group-uniform
                const int b = __ffsll((long long)m_live) - 1;
                m_live &= m_live - 1;
                const int got = __shfl(mine, gbase + b, 64);
                const int f = got >= 0 ? 1 : 0;
                const int64_t c = f ? got : ~got;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (role_sel(M, r) == 1) continue;
                    if (role_sel(M, r) == csel) {
                        const int d = role_dim<M>(m, r);
                        load_row_nomask<G, NCH>(R.x[r], m.tab[role_tab(M, r)] + c * (int64_t)d, d, gl);
                    }
                }
                const float s = model_fwd<M, G, NCH>(R, m, sv);
                if (first) {
                    s_true = s;
                } else {
                    const int lt = s < s_true ? 1 : 0, eq = s == s_true ? 1 : 0;   // a NaN compares false both ways
                    c_lt += lt; c_flt += lt & f; c_eq += eq; c_feq += eq & f;
                }
            }
        }
        if (gl == 0) {
            if (c_lt) atomicAdd(a.counts + q, c_lt);
            if (c_flt) atomicAdd(a.counts + (int64_t)n + q, c_flt);
            if (c_eq) atomicAdd(a.counts + 2 * (int64_t)n + q, c_eq);
            if (c_feq) atomicAdd(a.counts + 3 * (int64_t)n + q, c_feq);
        }
    }
}

// one wave per segment of candidate scores
template <typename T>
__global__ void __launch_bounds__(kBlock) k_rank_lists_from_scores(const T* __restrict__ scores, const T* __restrict__ truth,
                                                                   const int64_t* __restrict__ seg_off, int64_t n,
                                                                   const uint8_t* __restrict__ flags, int largest,
                                                                   int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const T st = truth[i];
    int c[4] = {0, 0, 0, 0};
    for (int64_t j = seg_off[i] + lane; j < seg_off[i + 1]; j += 64) {
        const T s = scores[j];
        const int f = flags ? flags[j] : 3;
        const int better = (largest ? s > st : s < st) ? 1 : 0, eq = s == st ? 1 : 0;
        const int live = f & 1, kept = (f >> 1) & f & 1;
        c[0] += better & live; c[1] += better & kept; c[2] += eq & live; c[3] += eq & kept;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
        if (lane == 0) counts[k * n + i] = c[k];
    }
}

static int launch_rank_candidates(const kge_model_desc* m, Geometry geo, const CandArgs* a, hipStream_t s) {
    const DeviceModel dm = to_device_model(m);
    KGE_DISPATCH_ROW_MODELS(m->model, (k_rank_candidates<M, G, NCH><<<dim3(kMaxBlocks), dim3(kBlock), 0, s>>>(dm, a)))
    set_error("kge_rank_candidates: unsupported model %d", m->model);
    return -1;
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_rank_candidates_workspace_bytes(int64_t n, int64_t n_lists, int64_t n_cand_ids) {
    (void)n_lists; (void)n_cand_ids;   // the item offsets are per query; the lists themselves are read in place
    if (n <= 0) return 0;
    return align256(sizeof(CandArgs)) + align256((size_t)(n + 1) * sizeof(int64_t)) + 256;   // + 256: the caller's pointer is aligned up
}

int kge_rank_candidates(const kge_model_desc* m, const int64_t* triples, int64_t n, int32_t side, const int64_t* list_of_query,
                        const int64_t* cand_off, const int32_t* cand_ids, int64_t n_lists, const int64_t* skip_off,
                        const int32_t* skip_ids, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream) {
    const char* who = "kge_rank_candidates";
    if (side != 0 && side != 1) { set_error("%s: side = %d (0 ranks tails, 1 ranks heads)", who, (int)side); return -1; }
    if (list_of_query && n_lists <= 0) { set_error("%s: list_of_query given with n_lists = %lld", who, (long long)n_lists); return -1; }
    if (!list_of_query && n_lists < n) { set_error("%s: n_lists = %lld < n = %lld without list_of_query", who, (long long)n_lists, (long long)n); return -1; }
    Geometry geo;
    const int go = rank_entry_checks(who, m, n, skip_off, skip_ids, workspace, workspace_bytes, kge_rank_candidates_workspace_bytes(n, n_lists, 0),
                                     "score the expanded live triples with the model's own forward and count with "
                                     "kge_rank_lists_from_scores (Evaluator.rank_candidates does)", &geo);
    if (go != kRankGo) return go;
    if (!triples || !cand_off || !cand_ids || !counts) { set_error("%s: null triples / cand_off / cand_ids / counts", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (list_of_query)
        if (int rc = debug_check_ids(who, "list_of_query", list_of_query, n, 1, 0, n_lists, s)) return rc;
    if (int rc = rank_counts_begin(who, m, triples, n, skip_off, skip_ids, counts, s)) return rc;
    CandArgs* args = (CandArgs*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);   // the kernel's copy of `a`, written by k_cand_items
    int64_t* item_off = (int64_t*)((char*)args + align256(sizeof(CandArgs)));
    const CandArgs a{triples, n, (int)side, list_of_query, cand_off, cand_ids, n_lists, skip_off, skip_ids, item_off, m->tot_entity, counts};
    hipLaunchKernelGGL(k_cand_items, dim3(1), dim3(kItemsBlock), 0, s, a, item_off, args);
    if (int rc = check_launch("k_cand_items")) return rc;
    return launch_rank_candidates(m, geo, args, s);
}

int kge_rank_lists_from_scores(const void* scores, int dtype, const void* truth_scores, const int64_t* seg_off, int64_t n,
                               const uint8_t* flags, int largest, int32_t* counts, void* stream) {
    const char* who = "kge_rank_lists_from_scores";
    if (dtype != 0 && dtype != 1) { set_error("%s: dtype = %d (0 = float32, 1 = float64)", who, dtype); return -1; }
    if (n < 0 || n > 0x7fffffffll) { set_error("%s: n = %lld outside 0..2^31-1", who, (long long)n); return -1; }
    if (n == 0) return 0;
    if (!scores || !truth_scores || !seg_off || !counts) { set_error("%s: null scores / truth_scores / seg_off / counts", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + kBlock / 64 - 1) / (kBlock / 64)));
    if (dtype == 0)
        hipLaunchKernelGGL((k_rank_lists_from_scores<float>), grid, dim3(kBlock), 0, s, (const float*)scores, (const float*)truth_scores,
                           seg_off, n, flags, largest ? 1 : 0, counts);
    else
        hipLaunchKernelGGL((k_rank_lists_from_scores<double>), grid, dim3(kBlock), 0, s, (const double*)scores, (const double*)truth_scores,
                           seg_off, n, flags, largest ? 1 : 0, counts);
    return check_launch("k_rank_lists_from_scores");
}

}  // extern "C"
