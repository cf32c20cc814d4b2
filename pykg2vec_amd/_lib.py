"""ctypes binding of libkge_hip.so (C ABI in include/kge_hip.h).

The HIP library IS the product path: if it is missing or a call fails this module raises -- there is no
CPU / PyTorch fallback anywhere in `pykg2vec_amd`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KGE_HIP_LIB", os.path.join(_HERE, "libkge_hip.so"))  # env override: A/B builds in dev tools

KGE_MAX_TABLES = 12
ABI_VERSION = 3

# enum kge_model
(TRANSE, TRANSH, TRANSD, ROTATE, RESCAL, NTN, DISTMULT, COMPLEX, ANALOGY, TRANSM, CP, SIMPLE, SIMPLE_IGNR,
 QUATE, TRANSR, SLM, SME, SME_BL, KG2E, HOLE, OCTONIONE) = range(21)
FLAG_L1 = 1
OPT_SGD, OPT_ADAM, OPT_ADAGRAD, OPT_RMSPROP = range(4)
REG_NONE, REG_F2, REG_N3, REG_N3_ABS, REG_ID_F2, REG_ID_N3 = range(6)
LOSS_SLOTS, LOSS_STRIDE = 32, 32  # loss accumulators: float[32*32], total = sum of [k*32]

c_i64p = ctypes.c_void_p  # all device pointers travel as void*


class ModelDesc(ctypes.Structure):
    """struct kge_model_desc"""
    _fields_ = [
        ("model", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("tot_entity", ctypes.c_int64),
        ("tot_relation", ctypes.c_int64),
        ("dim", ctypes.c_int32),
        ("rel_dim", ctypes.c_int32),
        ("margin", ctypes.c_float),
        ("phase_scale", ctypes.c_float),
        ("tables", ctypes.c_void_p * KGE_MAX_TABLES),
        ("grads", ctypes.c_void_p * KGE_MAX_TABLES),
    ]


class PullLists(ctypes.Structure):
    """struct kge_pull_lists"""
    _fields_ = [("pc", ctypes.c_void_p), ("count", ctypes.c_void_p), ("bucket", ctypes.c_void_p), ("head", ctypes.c_void_p),
                ("next", ctypes.c_void_p), ("sdesc", ctypes.c_void_p), ("dbucket", ctypes.c_void_p)]


PULL_BUCKET = 16


class PullBatch(ctypes.Structure):
    """struct kge_pull_batch"""
    _fields_ = [("pairs", ctypes.c_void_p), ("items", ctypes.c_void_p), ("n_items", ctypes.c_int64), ("dense_skip", ctypes.c_void_p),
                ("inc", ctypes.c_void_p), ("inv", ctypes.c_void_p),
                ("multi", ctypes.c_void_p), ("n_multi", ctypes.c_int64), ("n_pairs", ctypes.c_int64)]


class PullDirection(ctypes.Structure):
    """struct kge_pull_direction"""
    _fields_ = [("codes", ctypes.c_void_p), ("recs", ctypes.c_void_p), ("n_pairs", ctypes.c_int64),
                ("lists_without_descriptors", ctypes.c_int32)]


class PullPlanC(ctypes.Structure):
    """struct kge_pull_plan"""
    _fields_ = [("model", ModelDesc * 2), ("hat", (ctypes.c_void_p * 2) * 2), ("norm", ctypes.c_void_p * 2),
                ("state1", ctypes.c_void_p * 2), ("state2", ctypes.c_void_p * 2), ("lists", PullLists * 2),
                ("batches", ctypes.POINTER(PullBatch)), ("n_batches", ctypes.c_int64), ("partials", ctypes.c_void_p),
                ("margin", ctypes.c_float), ("optimizer", ctypes.c_int32), ("lr", ctypes.c_float),
                ("bern_prob", ctypes.c_void_p), ("slots", ctypes.c_void_p), ("n_slots", ctypes.c_int64),
                ("seed", ctypes.c_uint64), ("draws_per_batch", ctypes.c_int64), ("loss", ctypes.c_void_p),
                ("direction", PullDirection)]

class TransXPlanC(ctypes.Structure):
    """struct kge_transx_plan"""
    _fields_ = [("model", ModelDesc), ("lists", PullLists * 2), ("batches", ctypes.POINTER(PullBatch)), ("n_batches", ctypes.c_int64),
                ("partials", ctypes.c_void_p), ("stage", ctypes.c_void_p), ("recs", ctypes.c_void_p), ("margin", ctypes.c_float),
                ("flat_param", ctypes.c_void_p), ("flat_grad", ctypes.c_void_p), ("flat_state1", ctypes.c_void_p),
                ("flat_state2", ctypes.c_void_p), ("flat_numel", ctypes.c_int64), ("optimizer", ctypes.c_int32), ("lr", ctypes.c_float),
                ("bern_prob", ctypes.c_void_p), ("slots", ctypes.c_void_p), ("n_slots", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("draws_per_batch", ctypes.c_int64), ("loss", ctypes.c_void_p)]


class OwnPlanC(ctypes.Structure):
    """struct kge_own_plan"""
    _fields_ = [("model", ModelDesc), ("state1", ctypes.c_void_p * KGE_MAX_TABLES), ("state2", ctypes.c_void_p * KGE_MAX_TABLES),
                ("lists", PullLists * 2), ("batches", ctypes.POINTER(PullBatch)), ("n_batches", ctypes.c_int64),
                ("partials", ctypes.c_void_p), ("optimizer", ctypes.c_int32), ("lr", ctypes.c_float), ("lmbda", ctypes.c_float),
                ("reg_type", ctypes.c_int32), ("bern_prob", ctypes.c_void_p), ("slots", ctypes.c_void_p), ("n_slots", ctypes.c_int64),
                ("seed", ctypes.c_uint64), ("draws_per_batch", ctypes.c_int64), ("loss", ctypes.c_void_p), ("stage", ctypes.c_void_p)]


class RescalStage(ctypes.Structure):
    """struct kge_rescal_stage"""
    _fields_ = [("gstage", ctypes.c_void_p), ("dsv", ctypes.c_void_p), ("count", ctypes.c_void_p), ("bucket", ctypes.c_void_p),
                ("head", ctypes.c_void_p), ("next", ctypes.c_void_p), ("cap", ctypes.c_int32)]


class StagedTable(ctypes.Structure):
    """struct kge_staged_table"""
    _fields_ = [("cls", ctypes.c_int32), ("site_a", ctypes.c_int32), ("site_b", ctypes.c_int32), ("dsite", ctypes.c_int32),
                ("flat_off", ctypes.c_int64), ("rows", ctypes.c_int64)]


class StagedStep(ctypes.Structure):
    """struct kge_staged_step"""
    _fields_ = [("param", ctypes.c_void_p), ("state1", ctypes.c_void_p), ("state2", ctypes.c_void_p),
                ("tables", StagedTable * 8), ("n_tables", ctypes.c_int32), ("dim", ctypes.c_int32),
                ("ent_off", ctypes.c_void_p), ("ent_inc", ctypes.c_void_p), ("rel_off", ctypes.c_void_p), ("rel_inc", ctypes.c_void_p),
                ("rel_chunk_off", ctypes.c_void_p), ("chunk_rel", ctypes.c_void_p), ("rel_partials", ctypes.c_void_p),
                ("n_chunks", ctypes.c_int32),
                ("dyn_count", ctypes.c_void_p), ("dyn_bucket", ctypes.c_void_p), ("dyn_head", ctypes.c_void_p),
                ("dyn_next", ctypes.c_void_p), ("dyn_cap", ctypes.c_int32),
                ("dyn_count_next", ctypes.c_void_p), ("dyn_head_next", ctypes.c_void_p),
                ("touched_ent", ctypes.c_void_p), ("n_touched_ent", ctypes.c_int32), ("touched_rel", ctypes.c_void_p),
                ("n_touched_rel", ctypes.c_int32), ("dyn_list", ctypes.c_void_p),
                ("dyn_scale", ctypes.c_void_p),
                ("stage", ctypes.c_void_p), ("stage_stride", ctypes.c_int64),
                ("static_slots", ctypes.c_int32), ("dynamic_slots", ctypes.c_int32),
                ("n_pos", ctypes.c_int64), ("n_neg", ctypes.c_int64),
                ("tot_entity", ctypes.c_int64), ("tot_relation", ctypes.c_int64), ("stage_spare", ctypes.c_int32)]


CONVKB_MAX_WIDTHS = 8
TOPK_MAX = 1024   # KGE_TOPK_MAX: the most candidates kge_topk_rows returns per row
KNN_MAX = 128     # KGE_KNN_MAX: the most neighbours kge_knn_rows returns per query
KNN_METRICS = {"dot": 0, "cosine": 1, "l2": 2}   # KGE_KNN_DOT / _COSINE / _L2
TSNE_TILE = 256   # KGE_TSNE_TILE: points per tile of the t-SNE repulsion sweep
CAND_CHUNK = 64   # KGE_CAND_CHUNK: list entries per work item of kge_rank_candidates
REL_CHUNK = 64    # KGE_REL_CHUNK: relation ids per work item of kge_rank_relations
TYPED_ATTEMPTS = 16           # KGE_TYPED_ATTEMPTS: typed draws of kge_corrupt_typed before it falls back
TYPED_UNIFORM_ATTEMPTS = 64   # KGE_TYPED_UNIFORM_ATTEMPTS: uniform draws after those, then the row fails


class ConvKBDesc(ctypes.Structure):
    """struct kge_convkb_desc"""
    _fields_ = [("tot_entity", ctypes.c_int64), ("tot_relation", ctypes.c_int64), ("dim", ctypes.c_int32),
                ("num_filters", ctypes.c_int32), ("n_widths", ctypes.c_int32), ("widths", ctypes.c_int32 * CONVKB_MAX_WIDTHS),
                ("ent", ctypes.c_void_p), ("rel", ctypes.c_void_p), ("fc_w", ctypes.c_void_p), ("fc_b", ctypes.c_void_p),
                ("conv_w", ctypes.c_void_p), ("conv_b", ctypes.c_void_p), ("g_ent", ctypes.c_void_p), ("g_rel", ctypes.c_void_p),
                ("g_fc_w", ctypes.c_void_p), ("g_fc_b", ctypes.c_void_p)]


_CKB = ctypes.POINTER(ConvKBDesc)


class MurpDesc(ctypes.Structure):
    """struct kge_murp_desc (tables / grads: wu, bs, bo, ent, rel -- float64)"""
    _fields_ = [("tot_entity", ctypes.c_int64), ("tot_relation", ctypes.c_int64), ("dim", ctypes.c_int32), ("rank_order", ctypes.c_int32),
                ("tables", ctypes.c_void_p * 5), ("grads", ctypes.c_void_p * 5)]


_MRP = ctypes.POINTER(MurpDesc)


class TuckerDesc(ctypes.Structure):
    """struct kge_tucker_desc"""
    _fields_ = [("tot_entity", ctypes.c_int64), ("tot_relation", ctypes.c_int64), ("d1", ctypes.c_int32), ("d2", ctypes.c_int32),
                ("input_dropout", ctypes.c_float), ("hidden_dropout1", ctypes.c_float), ("hidden_dropout2", ctypes.c_float),
                ("train", ctypes.c_int32), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("ent", ctypes.c_void_p), ("rel", ctypes.c_void_p), ("W", ctypes.c_void_p),
                ("g_ent", ctypes.c_void_p), ("g_rel", ctypes.c_void_p), ("g_W", ctypes.c_void_p)]


_TKD = ctypes.POINTER(TuckerDesc)

PROJE_TABLES = ("ent", "rel", "bc1", "De1", "Dr1", "bc2", "De2", "Dr2")   # parameter_list order of ProjE_pointwise


class ProjeDesc(ctypes.Structure):
    """struct kge_proje_desc"""
    _fields_ = [("tot_entity", ctypes.c_int64), ("tot_relation", ctypes.c_int64), ("dim", ctypes.c_int32),
                ("hidden_dropout", ctypes.c_float), ("train", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64)] \
        + [(n, ctypes.c_void_p) for n in PROJE_TABLES] + [("g_" + n, ctypes.c_void_p) for n in PROJE_TABLES]


_PJD = ctypes.POINTER(ProjeDesc)

# ConvE's 13 parameters in state-dict (= descriptor) order, and its six running buffers
CONVE_TABLES = ("ent", "rel", "b", "bn0_w", "bn0_b", "conv_w", "conv_b", "bn1_w", "bn1_b", "fc_w", "fc_b", "bn2_w", "bn2_b")
CONVE_BUFFERS = ("bn0_mean", "bn0_var", "bn1_mean", "bn1_var", "bn2_mean", "bn2_var")
CONVE_MAX_HIDDEN = 1024


def _conv_1n_fields(geometry, tables, pad=False, index_tables=()):
    """The _fields_ of a conv 1-N descriptor (ConvE, HypER, InteractE, AcrE): the model's geometry, then the part the four structs
    share -- three dropout rates, train (and a reserved int32 where the geometry leaves seed misaligned), seed, offset, eps[3],
    momentum[3] -- then the index tables (InteractE's permutations), the tables, the six running buffers and the tables' gradients."""
    return [("tot_entity", ctypes.c_int64), ("tot_relation", ctypes.c_int64)] + [(n, ctypes.c_int32) for n in geometry] \
        + [(n, ctypes.c_float) for n in ("input_dropout", "feature_map_dropout", "hidden_dropout")] \
        + [("train", ctypes.c_int32)] + ([("reserved", ctypes.c_int32)] if pad else []) \
        + [("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("eps", ctypes.c_float * 3), ("momentum", ctypes.c_float * 3)] \
        + [(n, ctypes.c_void_p) for n in tuple(index_tables) + tuple(tables) + CONVE_BUFFERS] \
        + [("g_" + n, ctypes.c_void_p) for n in tables]


class ConveDesc(ctypes.Structure):
    """struct kge_conve_desc"""
    _fields_ = _conv_1n_fields(("hidden_size", "hidden_size_1"), CONVE_TABLES)


# HypER's 13 parameters in state-dict (= descriptor) order (the bare parameter b comes first), and its six running buffers
HYPER_TABLES = ("b", "ent", "rel", "bn0_w", "bn0_b", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "fc_w", "fc_b", "fc1_w", "fc1_b")
HYPER_BUFFERS = CONVE_BUFFERS
HYPER_MAX_HIDDEN = 1024


class HyperDesc(ctypes.Structure):
    """struct kge_hyper_desc"""
    _fields_ = _conv_1n_fields(("ent_hidden_size", "rel_hidden_size"), HYPER_TABLES)


# InteractE's 12 parameters in state-dict (= descriptor) order (the bare parameters bias and conv_filt come first), and its six buffers
INTERACTE_TABLES = ("bias", "conv_filt", "ent", "rel", "bn0_w", "bn0_b", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "fc_w", "fc_b")
INTERACTE_BUFFERS = CONVE_BUFFERS
INTERACTE_MAX_HIDDEN = 512
INTERACTE_MAX_KERNEL = 11
INTERACTE_MAX_FLAT = 1 << 22


class InteracteDesc(ctypes.Structure):
    """struct kge_interacte_desc"""
    _fields_ = _conv_1n_fields(("reshape_height", "reshape_width", "feature_permutation", "num_filters", "kernel_size"), INTERACTE_TABLES,
                               pad=True, index_tables=("perm", "inv_perm"))


# AcrE's parameters in state-dict (= descriptor) order (the bare parameter bias comes first): 17 in the serial way, 19 in the parallel
# (the gate); the descriptor has all 19 slots, the conv biases NULL without acre_bias and the gate NULL in the serial way
ACRE_TABLES_SERIAL = ("bias", "ent", "rel", "bn0_w", "bn0_b", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "fc_w", "fc_b", "conv1_w", "conv1_b",
                      "conv2_w", "conv2_b", "conv3_w", "conv3_b")
ACRE_TABLES_PARALLEL = ACRE_TABLES_SERIAL + ("gate_w", "gate_b")
ACRE_BUFFERS = CONVE_BUFFERS
ACRE_MAX_CHANNELS = 32
ACRE_MAX_ATROUS = 4


class AcreDesc(ctypes.Structure):
    """struct kge_acre_desc"""
    _fields_ = _conv_1n_fields(("hidden_size", "in_channels", "way", "first_atrous", "second_atrous", "third_atrous", "acre_bias"),
                               ACRE_TABLES_PARALLEL, pad=True)


_P, _I64 = ctypes.c_void_p, ctypes.c_int64


def _conv_1n_signatures(stem, desc, has_side=False):
    """The nine entry points of a 1-N model with its own descriptor (include/kge_hip.h: kge_<stem>_*).  has_side: ConvE's int32 side
    in front of row0 in the two body calls."""
    d = ctypes.POINTER(desc)
    body = (ctypes.c_int, [d, _P, _P, _I64] + [ctypes.c_int32] * has_side + [_I64, _P, _P, _P, ctypes.c_size_t, _P])
    sigs = {"saved_floats": (ctypes.c_size_t, [d, _I64]),
            "body_forward": body,
            "body_backward": body,
            "train_bce": (ctypes.c_int, [d, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, ctypes.c_float, _P, ctypes.c_size_t, _P, _P]),
            "eval_ranks": (ctypes.c_int, [d, _P, _I64] + [_P] * 4 + [_P, ctypes.c_size_t, _P, _P, _P])}
    sizes = {"body_forward": 1, "body_backward": 1, "train_bce": 3, "eval_ranks": 1}     # the int64 arguments of *_workspace_bytes
    sigs.update({e + "_workspace_bytes": (ctypes.c_size_t, [d] + [_I64] * k) for e, k in sizes.items()})
    return {"kge_%s_%s" % (stem, e): sig for e, sig in sigs.items()}


_SIGNATURES = {
    **_conv_1n_signatures("interacte", InteracteDesc),
    **_conv_1n_signatures("acre", AcreDesc),
    **_conv_1n_signatures("hyper", HyperDesc),
    **_conv_1n_signatures("conve", ConveDesc, has_side=True),
    "kge_proje_body_forward_workspace_bytes": (ctypes.c_size_t, [_PJD, ctypes.c_int64]),
    "kge_proje_body_forward": (ctypes.c_int, [_PJD, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_proje_body_backward_workspace_bytes": (ctypes.c_size_t, [_PJD, ctypes.c_int64]),
    "kge_proje_body_backward": (ctypes.c_int, [_PJD, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_proje_label_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]),
    "kge_proje_label_loss": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_size_t] + [ctypes.c_void_p] * 4),
    "kge_proje_train_workspace_bytes": (ctypes.c_size_t, [_PJD] + [ctypes.c_int64] * 4),
    "kge_proje_train": (ctypes.c_int, [_PJD] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                                      ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t,
                                                                      ctypes.c_void_p, ctypes.c_void_p]),
    "kge_proje_eval_ranks_workspace_bytes": (ctypes.c_size_t, [_PJD, ctypes.c_int64]),
    "kge_proje_eval_ranks": (ctypes.c_int, [_PJD, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
                             + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_tucker_saved_floats": (ctypes.c_size_t, [_TKD, ctypes.c_int64]),
    "kge_tucker_body_forward_workspace_bytes": (ctypes.c_size_t, [_TKD, ctypes.c_int64]),
    "kge_tucker_body_forward": (ctypes.c_int, [_TKD, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_tucker_body_backward_workspace_bytes": (ctypes.c_size_t, [_TKD, ctypes.c_int64]),
    "kge_tucker_body_backward": (ctypes.c_int, [_TKD, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_tucker_train_bce_workspace_bytes": (ctypes.c_size_t, [_TKD, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "kge_tucker_train_bce": (ctypes.c_int, [_TKD] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_tucker_eval_ranks_workspace_bytes": (ctypes.c_size_t, [_TKD, ctypes.c_int64]),
    "kge_tucker_eval_ranks": (ctypes.c_int, [_TKD, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
                              + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_convkb_collapse_workspace_bytes": (ctypes.c_size_t, [_CKB]),
    "kge_convkb_collapse": (ctypes.c_int, [_CKB, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_convkb_score_forward_workspace_bytes": (ctypes.c_size_t, [_CKB, ctypes.c_int64]),
    "kge_convkb_score_forward": (ctypes.c_int, [_CKB] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                                               ctypes.c_size_t, ctypes.c_void_p]),
    "kge_convkb_score_backward_workspace_bytes": (ctypes.c_size_t, [_CKB, ctypes.c_int64]),
    "kge_convkb_score_backward": (ctypes.c_int, [_CKB] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                                                ctypes.c_size_t, ctypes.c_void_p]),
    "kge_convkb_train_logistic_workspace_bytes": (ctypes.c_size_t, [_CKB, ctypes.c_int64]),
    "kge_convkb_train_logistic": (ctypes.c_int, [_CKB] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                                                ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_convkb_train_logistic_sampled_workspace_bytes": (ctypes.c_size_t, [_CKB, ctypes.c_int64, ctypes.c_int32]),
    "kge_convkb_train_logistic_sampled": (ctypes.c_int, [_CKB, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                         ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                         ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_convkb_eval_ranks_workspace_bytes": (ctypes.c_size_t, [_CKB, ctypes.c_int64]),
    "kge_convkb_eval_ranks": (ctypes.c_int, [_CKB, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
                              + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_convkb_sweep_scores_side_workspace_bytes": (ctypes.c_size_t, [_CKB, ctypes.c_int64]),
    "kge_murp_score_forward": (ctypes.c_int, [_MRP] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_murp_score_backward": (ctypes.c_int, [_MRP] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_murp_train_bce": (ctypes.c_int, [_MRP] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_murp_rsgd_step": (ctypes.c_int, [_MRP, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p]),
    "kge_murp_eval_ranks_workspace_bytes": (ctypes.c_size_t, [_MRP, ctypes.c_int64]),
    "kge_murp_eval_ranks": (ctypes.c_int, [_MRP, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
                            + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_murp_sweep_scores_side_workspace_bytes": (ctypes.c_size_t, [_MRP, ctypes.c_int64]),
    "kge_murp_sweep_scores_side": (ctypes.c_int, [_MRP, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                  ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_convkb_sweep_scores_side": (ctypes.c_int, [_CKB, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                    ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_staged_step_bytes": (ctypes.c_size_t, []),
    "kge_train_pairwise_selfadv_sampled_staged": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                                  ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p,
                                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64,
                                                                  ctypes.POINTER(StagedStep), ctypes.c_void_p, ctypes.c_void_p]),
    "kge_train_pointwise_logistic_sampled_staged": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                                    ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                                    ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_float,
                                                                    ctypes.c_int32, ctypes.POINTER(StagedStep), ctypes.c_void_p,
                                                                    ctypes.c_void_p]),
    "kge_optimizer_step_staged": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(StagedStep), ctypes.c_float, ctypes.c_int64, ctypes.c_void_p]),
    "kge_abi_version": (ctypes.c_int, []),
    "kge_set_debug": (ctypes.c_int, [ctypes.c_int32]),
    "kge_set_switch": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32]),
    "kge_get_debug": (ctypes.c_int, []),
    "kge_check_ids": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "kge_debug_marker": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p]),
    "kge_filter_csr_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "kge_filter_csr_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_filter_csr_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_topk_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "kge_topk_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_knn_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int]),
    "kge_knn_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_tsne_affinities": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "kge_tsne_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "kge_tsne_gradient": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "kge_tsne_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_float,
                                    ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                    ctypes.c_size_t, ctypes.c_void_p]),
    "kge_rank_candidates_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "kge_rank_candidates": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_rank_lists_from_scores": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_rank_relations_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "kge_rank_relations": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_relation_csr_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "kge_relation_csr_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_relation_csr_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "kge_classification_sort_length": (ctypes.c_int64, [ctypes.c_int64]),
    "kge_classification_fit_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "kge_classification_fit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_classification_apply": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_corrupt_typed": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 3 + [ctypes.c_void_p] * 4
                          + [ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_last_error": (ctypes.c_char_p, []),
    "kge_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ModelDesc), ctypes.c_int64]),
    "kge_score_forward": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_score_backward": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_rescal_normalize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]),
    "kge_rescal_normalize_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32]),
    "kge_rescal_normalize_ws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "kge_train_pairwise_hinge": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_train_pairwise_hinge_sampled": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_train_pairwise_selfadv": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_train_pairwise_selfadv_sampled": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_train_pointwise_logistic": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_train_pointwise_logistic_sampled": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                            ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_float, ctypes.c_int32,
                                                            ctypes.c_void_p, ctypes.c_void_p]),
    "kge_l2norm_reg": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_head_1n_rank_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]),
    "kge_head_1n_rank": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_head_1n_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_head_1n_forward_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_head_1n_backward_workspace_bytes": (ctypes.c_size_t, []),
    "kge_head_1n_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]
                             + [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]),
    "kge_head_1n_bce_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "kge_head_1n_bce": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                       ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 5),
    "kge_optimizer_step": (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_float, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_optimizer_step_rows": (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_float,
                                               ctypes.c_int64, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 4),
    "kge_optimizer_step_rownorm_ok": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "kge_optimizer_step_rownorm": (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_int64,
                                                  ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "kge_optimizer_step_rows_rownorm": (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 4
                                        + [ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
                                        + [ctypes.c_void_p] * 3 + [ctypes.POINTER(RescalStage), ctypes.c_void_p, ctypes.c_size_t]
                                        + [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 3 + [ctypes.c_void_p]),
    "kge_rescal_pair_step": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_rescal_pair_step_ok": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_int64]),
    "kge_rescal_stage_ok": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_int64]),
    "kge_rescal_pair_step_staged": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                                   ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(RescalStage), ctypes.c_void_p]),
    "kge_optimizer_step_rows_staged": (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_float,
                                                      ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.POINTER(RescalStage), ctypes.c_void_p]),
    "kge_step_advance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]),
    "kge_optimizer_step_advance": (ctypes.c_int, [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_float, ctypes.c_int32]
                                   + [ctypes.c_void_p] * 4 + [ctypes.c_int64] * 3 + [ctypes.c_void_p]),
    "kge_eval_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ModelDesc), ctypes.c_int64]),
    "kge_eval_ranks": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_eval_ranks_ties": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_eval_ranks_grouped_ties": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
                                    + [ctypes.c_void_p] * 4 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_eval_grouped_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(ModelDesc), ctypes.c_int64, ctypes.c_int64]),
    "kge_eval_ranks_grouped": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
                               + [ctypes.c_void_p] * 4 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_eval_sweep_scores": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_eval_sweep_scores_side": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_rank_from_scores": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_void_p]),
    "kge_triple_set_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "kge_corrupt": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [ctypes.c_void_p]),
    "kge_sample_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32] + [ctypes.c_void_p] * 6 + [ctypes.c_void_p, ctypes.c_void_p]),
    "kge_pull_partial_stride": (ctypes.c_int, [ctypes.c_int32]),
    "kge_pull_hat_stride": (ctypes.c_int, [ctypes.c_int32]),
    "kge_pull_groups_per_block": (ctypes.c_int, [ctypes.c_int32]),
    "kge_row_norms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_pull_sample": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(PullLists), ctypes.c_void_p]),
    "kge_pull_lists_explicit": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.POINTER(PullLists), ctypes.c_void_p]),
    "kge_pull_step": (ctypes.c_int, [ctypes.POINTER(ModelDesc)] + [ctypes.c_void_p] * 8 + [ctypes.POINTER(PullLists), ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float,
                                     ctypes.c_int32, ctypes.c_float, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(PullLists), ctypes.c_void_p,
                                     ctypes.POINTER(PullDirection), ctypes.c_void_p]),
    "kge_pull_direction_bytes": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t),
                                                ctypes.POINTER(ctypes.c_size_t)]),
    "kge_transx_groups_per_block": (ctypes.c_int, [ctypes.c_int32]),
    "kge_transx_partial_stride": (ctypes.c_int, [ctypes.c_int32]),
    "kge_transx_scratch_bytes": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t),
                                                ctypes.POINTER(ctypes.c_size_t)]),
    "kge_transx_grad_step": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(PullLists), ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(PullLists), ctypes.c_void_p, ctypes.c_void_p]),
    "kge_transx_plan_bytes": (ctypes.c_size_t, []),
    "kge_transx_run": (ctypes.c_int, [ctypes.POINTER(TransXPlanC), ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]),
    "kge_own_groups_per_block": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32]),
    "kge_own_partial_stride": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32]),
    "kge_own_stage_bytes": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    "kge_own_step": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(PullLists), ctypes.c_void_p,
                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_float,
                                    ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(PullLists),
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kge_own_apply": (ctypes.c_int, [ctypes.POINTER(ModelDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.POINTER(PullLists), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int64,
                                     ctypes.c_void_p]),
    "kge_own_plan_bytes": (ctypes.c_size_t, []),
    "kge_own_run": (ctypes.c_int, [ctypes.POINTER(OwnPlanC), ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]),
    "kge_pull_index_geometry": (ctypes.c_int, [ctypes.c_int64] * 4 + [ctypes.c_int32] * 3 + [ctypes.POINTER(ctypes.c_int64)] * 3
                                + [ctypes.POINTER(ctypes.c_size_t)]),
    "kge_pull_index_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int64] * 6 + [ctypes.c_int32] * 3
                             + [ctypes.c_void_p] * 8 + [ctypes.c_size_t, ctypes.c_void_p]),
    "kge_pull_plan_bytes": (ctypes.c_size_t, []),
    "kge_pull_run": (ctypes.c_int, [ctypes.POINTER(PullPlanC), ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class KgeHipError(RuntimeError):
    pass


def load():
    """Load libkge_hip.so (once).  Raises if it has not been built: build with
    `python -c 'import __graft_entry__ as g; g.build()'` or `make -C pykg2vec_amd/csrc`."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KgeHipError("libkge_hip.so not found at %s -- the HIP extension is mandatory (no CPU fallback); "
                          "run __graft_entry__.build()" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.kge_abi_version() != ABI_VERSION:
        raise KgeHipError("libkge_hip.so ABI %d != expected %d" % (lib.kge_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().kge_last_error()
        raise KgeHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
