// kge_projection.hip -- the rank pass and the small host checks shared by the 1-N models with their own descriptor (kge_projection.h,
// DESIGN.md section 17).  A model's kge_*_eval_ranks checks its descriptor, fills a ProjectionEval and calls projection_eval_ranks.
#include "kge_projection.h"

namespace kge {

// the rank pass's glue: the rows [h; t] with their relations, triples with the true entity of the head sweep in column 2, and the
// [4, n] layout of kge_eval_ranks
__global__ void k_projection_eval_ids(const int64_t* __restrict__ triples, int64_t n, int64_t* __restrict__ e, int64_t* __restrict__ r,
                                      int64_t* __restrict__ swapped) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t h = triples[3 * i], rel = triples[3 * i + 1], t = triples[3 * i + 2];
    e[i] = h; e[n + i] = t;
    __builtin_amdgcn_sched_barrier(0);   // (the addresses of the stores below are formed after these two: 15 VGPRs, not 17)
    r[i] = rel; r[n + i] = rel;
    swapped[3 * i] = t; swapped[3 * i + 1] = rel; swapped[3 * i + 2] = h;
}
__global__ void k_projection_pack_ranks(const int32_t* __restrict__ tail, const int32_t* __restrict__ head, int64_t n,
                                        int32_t* __restrict__ ranks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ranks[i] = head[i];
    ranks[n + i] = tail[i];
    ranks[2 * n + i] = head[n + i];
    ranks[3 * n + i] = tail[n + i];
}

int ws_check(const char* who, const void* ws, size_t have, size_t need) {
    if (!ws || have < need) { set_error("%s: workspace too small (%zu < %zu bytes)", who, ws ? have : (size_t)0, need); return -1; }
    return 0;
}

int check_er_ids(const char* who, int64_t tot_entity, int64_t tot_relation, const int64_t* e, const int64_t* r, int64_t n, hipStream_t s) {
    if (int rc = debug_check_ids(who, "entity", e, n, 1, 0, tot_entity, s)) return rc;
    return debug_check_ids(who, "relation", r, n, 1, 0, tot_relation, s);
}

// rank: ids e [2n] r [2n] | swapped triples [3n int64] | x [2n, dim] | ranks of the two sweeps [2 x 2n int32] | max(body, head rank)
struct ProjectionEvalPlan {
    size_t ids, swapped, x, ranks, rest, total;
};
static ProjectionEvalPlan projection_eval_plan(const ProjectionEval& m, int64_t n) {
    ProjectionEvalPlan p{};
    p.ids = 0;
    p.swapped = align256((size_t)4 * n * sizeof(int64_t));
    p.x = p.swapped + align256((size_t)3 * n * sizeof(int64_t));
    p.ranks = p.x + align256((size_t)2 * n * m.dim * sizeof(float));
    p.rest = p.ranks + align256((size_t)4 * n * sizeof(int32_t));
    size_t rest = m.body_bytes;
    const size_t hr = kge_head_1n_rank_workspace_bytes(n, m.dim, m.tot_entity, m.bias ? 1 : 0);
    if (hr > rest) rest = hr;
    p.total = p.rest + align256(rest);
    return p;
}

size_t projection_eval_workspace_bytes(const ProjectionEval& m, int64_t n) { return projection_eval_plan(m, n > 0 ? n : 1).total; }

int projection_eval_ranks(const char* who, const ProjectionEval& m, const void* desc, const int64_t* triples, int64_t n,
                          const int64_t* tail_off, const int32_t* tail_ids, const int64_t* head_off, const int32_t* head_ids, void* workspace,
                          size_t workspace_bytes, int32_t* ranks, int32_t* ties, void* stream) {
    if (n < 0 || (n > 0 && (!triples || !ranks)) || (tail_off && !tail_ids) || (head_off && !head_ids)) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    const ProjectionEvalPlan p = projection_eval_plan(m, n > 0 ? n : 1);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = debug_check_triples(who, m.tot_entity, m.tot_relation, triples, n, s)) return rc;
    char* ws = (char*)workspace;
    int64_t* e = (int64_t*)(ws + p.ids);
    int64_t* rr = e + 2 * n;
    int64_t* swapped = (int64_t*)(ws + p.swapped);
    float* x = (float*)(ws + p.x);
    int32_t* tmp = (int32_t*)(ws + p.ranks);
    void* rest = ws + p.rest;
    const size_t rest_bytes = p.total - p.rest;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_projection_eval_ids, dim3(blocks), dim3(256), 0, s, triples, n, e, rr, swapped);
    if (int rc = check_launch("k_projection_eval_ids")) return rc;
    if (int rc = m.body(desc, e, rr, n, x, rest, rest_bytes, s)) return rc;
    // tail sweep: body(h, r), true entity t, filter hr_t; head sweep: body(t, r), true entity h, filter tr_h
    if (int rc = kge_head_1n_rank(x, n, m.dim, m.ent, m.tot_entity, m.bias, triples, tail_off, tail_ids, rest, rest_bytes, tmp,
                                  ties ? ties + n : nullptr, nullptr, stream)) return rc;
    if (int rc = kge_head_1n_rank(x + n * m.dim, n, m.dim, m.ent, m.tot_entity, m.bias, swapped, head_off, head_ids, rest, rest_bytes,
                                  tmp + 2 * n, ties, nullptr, stream)) return rc;
    hipLaunchKernelGGL(k_projection_pack_ranks, dim3(blocks), dim3(256), 0, s, tmp, tmp + 2 * n, n, ranks);
    return check_launch("k_projection_pack_ranks");
}

}  // namespace kge
