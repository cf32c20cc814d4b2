// kge_models.hip -- the per-model table (ModelOps, kge_internal.h): which launchers serve which kge_model id.  Host code only.
// Adding a model: one row here, in id order, plus its launchers (declared with the table's function types in kge_internal.h);
// a field left NULL takes the default named beside it in ModelOps.
#include "kge_internal.h"

namespace kge {

struct ModelRow { int model; ModelOps ops; };

#define KGE_NO_SCORER nullptr, nullptr, nullptr, nullptr, nullptr, nullptr
#define KGE_ROWS(T, G) {T, G, true, KGE_NO_SCORER, nullptr, nullptr}   /* gather / row kernels, generic rank pipeline */
#define KGE_SEMANTIC(T)                                                                                                              \
    {T, T, false, semantic_workspace_bytes, launch_semantic_forward, launch_semantic_backward, launch_semantic_pair_forward,        \
     launch_semantic_pair_backward, nullptr, semantic_eval_workspace_bytes, launch_semantic_eval}

//   id                tables, grads, row kernels, scorer workspace, forward, backward, pair forward, pair backward, pair fast, rank workspace, rank
static constexpr ModelRow kModels[] = {
    {KGE_TRANSE, KGE_ROWS(2, 2)},
    {KGE_TRANSH, KGE_ROWS(3, 3)},
    {KGE_TRANSD, KGE_ROWS(4, 4)},
    {KGE_ROTATE, KGE_ROWS(3, 3)},
    {KGE_RESCAL, {2, 2, false, rescal_workspace_bytes, launch_rescal_forward, launch_rescal_backward, launch_rescal_pair_forward,
                  launch_rescal_pair_backward, rescal_pair_fast, nullptr, nullptr}},
    {KGE_NTN, {6, 6, false, ntn_workspace_bytes, launch_ntn_forward, launch_ntn_backward, launch_ntn_pair_forward,
               launch_ntn_pair_backward, nullptr, ntn_eval_workspace_bytes, launch_ntn_eval}},
    {KGE_DISTMULT, KGE_ROWS(2, 2)},
    {KGE_COMPLEX, KGE_ROWS(4, 4)},
    {KGE_ANALOGY, KGE_ROWS(6, 6)},
    {KGE_TRANSM, KGE_ROWS(3, 2)},   // theta is a fixed input: no gradient buffer
    {KGE_CP, KGE_ROWS(3, 3)},
    {KGE_SIMPLE, KGE_ROWS(4, 4)},
    {KGE_SIMPLE_IGNR, KGE_ROWS(4, 4)},
    {KGE_QUATE, KGE_ROWS(8, 8)},
    {KGE_TRANSR, {3, 3, false, transr_workspace_bytes, launch_transr_forward, launch_transr_backward, launch_transr_pair_forward,
                  launch_transr_pair_backward, transr_pair_fast, nullptr, nullptr}},
    {KGE_SLM, KGE_SEMANTIC(4)},
    {KGE_SME, KGE_SEMANTIC(8)},
    {KGE_SME_BL, KGE_SEMANTIC(8)},
    {KGE_KG2E, {4, 4, true, KGE_NO_SCORER, kg2e_eval_workspace_bytes, launch_kg2e_eval}},
    {KGE_HOLE, {2, 2, false, nullptr, launch_hole_forward, launch_hole_backward, launch_hole_pair_forward, launch_hole_pair_backward,
                nullptr, hole_eval_workspace_bytes, launch_hole_eval}},
    // the entity and relation component blocks; trained by the pointwise logistic step only: no pair step
    {KGE_OCTONIONE, {2, 2, false, nullptr, launch_octonion_forward, launch_octonion_backward, nullptr, nullptr, nullptr,
                     octonion_eval_workspace_bytes, launch_octonion_eval}},
};
#undef KGE_SEMANTIC
#undef KGE_ROWS
#undef KGE_NO_SCORER

constexpr int kModelCount = (int)(sizeof(kModels) / sizeof(kModels[0]));
constexpr bool rows_in_id_order() {
    for (int i = 0; i < kModelCount; ++i)
        if (kModels[i].model != i) return false;
    return true;
}
static_assert(kModelCount == KGE_OCTONIONE + 1 && rows_in_id_order(), "kModels needs one row per kge_model id, in id order");

const ModelOps* model_ops(int model) { return model >= 0 && model < kModelCount ? &kModels[model].ops : nullptr; }

}  // namespace kge
