// kge_relations.hip -- relation ranking: for query i = (h, r, t), where does the true relation r stand among ALL relations r' of
// (h, r', t), raw and with the relations known for the pair (h, t) left out?  The relation side of the filtered link-prediction
// protocol; the reference only has the inference hook (utils/evaluator.py:275-287, test_rel_rank), no metric over it.
//
//   items    an item is (query, chunk of KGE_REL_CHUNK consecutive relation ids): item it belongs to query it / chunks and walks
//            the relations [(it % chunks) * KGE_REL_CHUNK, + KGE_REL_CHUNK) below R, chunks = ceil(R / KGE_REL_CHUNK).  Every query
//            has the same number of items, so the mapping is a division: no scan kernel, no offsets.  The grid strides over items.
//   kernel   k_rank_relations<M, G, NCH>, the row kernels' geometry (kge_row_kernels.h): one G-lane group per item.  The group loads
//            the query's entity-side rows (the roles whose id is NOT the relation, role_sel != 1) once.  It then walks entries:
//            first the true relation alone, whose score it keeps as s_true, then per step G relation ids.  In such a step every
//            lane takes one id and decides its liveness (below R, not the true relation; binary search in the query's ascending skip
//            segment: G searches in flight); a ballot gives the group the mask of live ids, and the id travels with "left out by the
//            filter" in its sign.  Per walked relation only the roles with role_sel == 1 are gathered (TransH's w, TransD's
//            projection row, TransM's theta, KG2E's mean and variance, SimplE's two, ANALOGY's three, QuatE's four), and model_fwd
//            runs on the same row values in the same geometry as k_score_fwd (-ffp-contract=off, no fast-math), so the compared scores
//            are kge_score_forward's bit for bit.  The relation tables are small (538 KB at R = 1345, d = 100): the walk reads L2.
//   counts   four integer counters per group, added with integer atomicAdd to counts [4, n], which a memset on the stream zeroed:
//            the result does not depend on the arrival order.
//   scalars  as kge_candidates.hip: rows are loaded without lane masks, the arguments are read from a workspace copy (written by
//            k_rel_args), and ONE walk loop serves the true relation and the others, so that model_fwd is instantiated once.  The
//            kernel is held to k_score_fwd's resources (tests/test_relations_resources.py).
//   shared   with kge_candidates.hip, in kge_rank_common.h: load_row_nomask, the list of row-kernel models, and the entry point's
//            opening (rank_entry_checks, rank_counts_begin).  The walk loop is not shared: DESIGN.md section 30.
#include "kge_rank_common.h"

namespace kge {

namespace {

constexpr int kRelChunk = KGE_REL_CHUNK;

struct RelArgs {
    const int64_t* triples; int64_t n;
    const int64_t* skip_off; const int32_t* skip_ids;
    int32_t* counts; int R; int chunks;
};

}  // namespace

// the kernel's copy of the call's arguments (field by field: a struct copy goes through a stack object)
__global__ void __launch_bounds__(64) k_rel_args(RelArgs a, RelArgs* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out->triples = a.triples; out->n = a.n; out->skip_off = a.skip_off; out->skip_ids = a.skip_ids;
    out->counts = a.counts; out->R = a.R; out->chunks = a.chunks;
}

template <int M, int G, int NCH>
__global__ __launch_bounds__(kBlock) void k_rank_relations(DeviceModel m, const RelArgs* args) {
    const RelArgs& a = *args;   // read where used: a few scalar loads per item instead of a dozen scalar registers for the whole kernel
    constexpr int GPB = kBlock / G;
    constexpr int NR = role_count(M);
    const int gl = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) / G * G;   // first lane of the group inside its wave
    const int64_t n = a.n;
    const int chunks = a.chunks;
    const int64_t n_items = n * chunks;
    for (int64_t it = (int64_t)blockIdx.x * GPB + threadIdx.x / G; it < n_items; it += (int64_t)gridDim.x * GPB) {
        const int64_t q = it / chunks;
        const int first_rel = (int)(it - q * chunks) * kRelChunk;
        const int cnt = min(a.R - first_rel, kRelChunk);   // >= 1: chunks = ceil(R / kRelChunk)
        const int64_t id[3] = {a.triples[3 * q], a.triples[3 * q + 1], a.triples[3 * q + 2]};
        const int truth = (int)id[1];
        const int32_t* skip = nullptr;   // the query's ascending skip segment: skip[0 .. n_skip)
        int n_skip = 0;
        if (a.skip_off) { skip = a.skip_ids + a.skip_off[q]; n_skip = (int)(a.skip_off[q + 1] - a.skip_off[q]); }
        Rows<M, NCH> R;   // the entity-side rows now; the relation's rows come per walked relation
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (role_sel(M, r) == 1) continue;
            const int d = role_dim<M>(m, r);
            load_row_nomask<G, NCH>(R.x[r], m.tab[role_tab(M, r)] + id[role_sel(M, r)] * (int64_t)d, d, gl);
        }
        Saved<M, NCH> sv;
        float s_true = 0.f;
        int c_lt = 0, c_flt = 0, c_eq = 0, c_feq = 0;
        // step -G walks ONE entry, the true relation, and keeps its score; the steps from 0 on take G relation ids each.  One walk
        // loop, so model_fwd is instantiated once per kernel.
        for (int base = -G; base < cnt; base += G) {
            const int j = base + gl;
            const bool first = base < 0;   // group-uniform
            const int e = first ? truth : first_rel + j;
            const bool live = first ? gl == 0 : (j < cnt && e != truth);
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
                    if (role_sel(M, r) != 1) continue;
                    const int d = role_dim<M>(m, r);
                    load_row_nomask<G, NCH>(R.x[r], m.tab[role_tab(M, r)] + c * (int64_t)d, d, gl);
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
            if (c_flt) atomicAdd(a.counts + n + q, c_flt);
            if (c_eq) atomicAdd(a.counts + 2 * n + q, c_eq);
            if (c_feq) atomicAdd(a.counts + 3 * n + q, c_feq);
        }
    }
}

static int launch_rank_relations(const kge_model_desc* m, Geometry geo, const RelArgs* a, int64_t n_items, hipStream_t s) {
    const DeviceModel dm = to_device_model(m);
    KGE_DISPATCH_ROW_MODELS(m->model, (k_rank_relations<M, G, NCH><<<dim3(Launch<M, G, NCH>::grid(n_items)), dim3(kBlock), 0, s>>>(dm, a)))
    set_error("kge_rank_relations: unsupported model %d", m->model);
    return -1;
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_rank_relations_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return align256(sizeof(RelArgs)) + 256;   // the kernel's copy of the arguments; + 256: the caller's pointer is aligned up
}

int kge_rank_relations(const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* skip_off, const int32_t* skip_ids,
                       void* workspace, size_t workspace_bytes, int32_t* counts, void* stream) {
    const char* who = "kge_rank_relations";
    if (m && m->tot_relation > 0x7fffffffll) {   // the walked ids are ints
        set_error("%s: bad sizes (dim %d, entities %lld, relations %lld)", who, m->dim, (long long)m->tot_entity, (long long)m->tot_relation);
        return -1;
    }
    Geometry geo;
    const int go = rank_entry_checks(who, m, n, skip_off, skip_ids, workspace, workspace_bytes, kge_rank_relations_workspace_bytes(n),
                                     "score the triples of every other relation with the model's own forward and count with "
                                     "kge_rank_lists_from_scores (Evaluator.rank_relations does)", &geo);
    if (go != kRankGo) return go;
    if (!triples || !counts) { set_error("%s: null triples / counts", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rank_counts_begin(who, m, triples, n, skip_off, skip_ids, counts, s)) return rc;
    RelArgs* args = (RelArgs*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int R = (int)m->tot_relation;
    const int chunks = (R + kRelChunk - 1) / kRelChunk;
    const RelArgs a{triples, n, skip_off, skip_ids, counts, R, chunks};
    hipLaunchKernelGGL(k_rel_args, dim3(1), dim3(64), 0, s, a, args);
    if (int rc = check_launch("k_rel_args")) return rc;
    return launch_rank_relations(m, geo, args, n * chunks, s);
}

}  // extern "C"
