// kge_rank_common.h -- what kge_candidates.hip and kge_relations.hip share: the unmasked row load of their walk loops, the list of
// models that have a walk kernel, and the host-side opening of their entry points.  The walk loops themselves stay one per kernel
// (DESIGN.md section 30 has the merge that was tried and what it cost in registers).
#pragma once
#include "kge_row_kernels.h"

namespace kge {

// load_row's values with no lane mask: a padding element reads the row's last float and is zeroed with an integer AND (+0.0, as
// load_row gives).  The e < dim tests of load_row are loop-invariant lane masks that the compiler keeps in scalar register pairs
// for the whole kernel, 2 * NCH of them; next to the walk kernels' arguments they no longer fit.
template <int G, int NCH>
__device__ __forceinline__ void load_row_nomask(float (&x)[NCH], const float* __restrict__ row, int dim, int gl) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int e = c * G + gl;
        int keep = (e - dim) >> 31;   // all ones where e < dim
        asm volatile("" : "+v"(keep));   // (opaque: otherwise it is folded back into a test, i.e. a lane mask)
        int ec = min(e, dim - 1);
        asm volatile("" : "+v"(ec));     // (opaque: redone per row, or NCH clamped indices stay live in vector registers)
        x[c] = __int_as_float(__float_as_int(row[ec]) & keep);
    }
}

// the models with row kernels (ModelOps::row_kernels): the ones k_rank_candidates / k_rank_relations are instantiated for
#define KGE_DISPATCH_ROW_MODELS(model_id, BODY)                 \
    switch (model_id) {                                         \
        KGE_FOR_MODEL(KGE_TRANSE, BODY)                         \
        KGE_FOR_MODEL(KGE_TRANSH, BODY)                         \
        KGE_FOR_MODEL(KGE_TRANSD, BODY)                         \
        KGE_FOR_MODEL(KGE_TRANSM, BODY)                         \
        KGE_FOR_MODEL(KGE_ROTATE, BODY)                         \
        KGE_FOR_MODEL(KGE_DISTMULT, BODY)                       \
        KGE_FOR_MODEL(KGE_COMPLEX, BODY)                        \
        KGE_FOR_MODEL(KGE_ANALOGY, BODY)                        \
        KGE_FOR_MODEL(KGE_CP, BODY)                             \
        KGE_FOR_MODEL(KGE_SIMPLE, BODY)                         \
        KGE_FOR_MODEL(KGE_SIMPLE_IGNR, BODY)                    \
        KGE_FOR_MODEL(KGE_QUATE, BODY)                          \
        KGE_FOR_MODEL(KGE_KG2E, BODY)                           \
        default: break;                                         \
    }

// The opening of kge_rank_candidates / kge_rank_relations: descriptor, row-kernel model, sizes, tables, range of n, the skip pair,
// the workspace (`need` = <who>_workspace_bytes), the geometry.  kRankRefused: kge_last_error is set, return -1; kRankNothing:
// n == 0, return 0 (what comes after the n == 0 test -- the geometry, the caller's null checks -- is not looked at then).
enum { kRankRefused = -1, kRankNothing = 0, kRankGo = 1 };
inline int rank_entry_checks(const char* who, const kge_model_desc* m, int64_t n, const int64_t* skip_off, const int32_t* skip_ids,
                             const void* workspace, size_t workspace_bytes, size_t need, const char* via_forward_hint, Geometry* geo) {
    if (!m) { set_error("%s: null model descriptor", who); return kRankRefused; }
    const ModelOps* ops = model_ops(m->model);
    if (!ops) { set_error("%s: unknown model id %d", who, m->model); return kRankRefused; }
    if (!ops->row_kernels) {
        set_error("%s: model %d has no row kernels; rank it via-forward: %s", who, m->model, via_forward_hint);
        return kRankRefused;
    }
    if (m->dim <= 0 || m->tot_entity <= 0 || m->tot_relation <= 0) {
        set_error("%s: bad sizes (dim %d, entities %lld, relations %lld)", who, m->dim, (long long)m->tot_entity, (long long)m->tot_relation);
        return kRankRefused;
    }
    for (int i = 0; i < ops->tables; ++i)
        if (!m->tables[i]) { set_error("%s: table %d is null", who, i); return kRankRefused; }
    if (n < 0 || n > 0x7fffffffll) { set_error("%s: n = %lld outside 0..2^31-1", who, (long long)n); return kRankRefused; }
    if ((skip_off == nullptr) != (skip_ids == nullptr)) { set_error("%s: skip_off and skip_ids come together", who); return kRankRefused; }
    if (n > 0 && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace too small (%zu bytes, %s_workspace_bytes asks for %zu)", who, workspace ? workspace_bytes : (size_t)0, who, need);
        return kRankRefused;
    }
    if (n == 0) return kRankNothing;
    if (!pick_geometry(m->dim, geo)) {
        set_error("%s: hidden size %d exceeds the register-resident row kernels (max 2048)", who, m->dim);
        return kRankRefused;
    }
    return kRankGo;
}

// the debug-mode scans of the queries and their skip segments, then counts [4, n] = 0 on the stream; 0 or the failing call's code
inline int rank_counts_begin(const char* who, const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* skip_off,
                             const int32_t* skip_ids, int32_t* counts, hipStream_t s) {
    if (int rc = debug_check_triples(who, m->tot_entity, m->tot_relation, triples, n, s)) return rc;
    if (skip_off)
        if (int rc = debug_check_ascending(who, "skip", skip_off, skip_ids, n, s)) return rc;
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)4 * (size_t)n * sizeof(int32_t), s);
    if (e != hipSuccess) { set_error("%s: memset: %s", who, hipGetErrorString(e)); return -2; }
    return 0;
}

}  // namespace kge
