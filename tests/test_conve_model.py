"""ConvE without a GPU: the float64 restatement (tools/conve_reference.py) reproduces the live reference's float64 outputs frozen in
tests/golden/ref_conve{,_ls,_masked}.npz (1e-10, ranks exact) and the recorded Philox masks; the drop-in class keeps the reference's
construction contract and state dict; every refusal that needs no device raises with its sentence; the ctypes struct agrees with the
header."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import conve_reference as cr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["conve", "conve_ls", "conve_masked"]
TENSORS, BUFFERS, COUNTERS = cr.TENSORS, cr.BUFFERS, cr.COUNTERS
PARAMS = dict(tot_entity=70, tot_relation=5, hidden_size=20, hidden_size_1=5, lmbda=0.1, input_dropout=0.2, feature_map_dropout=0.2,
              hidden_dropout=0.3)
SHAPES = {"ent_embeddings.weight": (70, 20), "rel_embeddings.weight": (10, 20), "b.weight": (1, 70),
          "bn0.weight": (1,), "bn0.bias": (1,), "bn0.running_mean": (1,), "bn0.running_var": (1,), "bn0.num_batches_tracked": (),
          "conv2d_1.weight": (32, 1, 3, 3), "conv2d_1.bias": (32,),
          "bn1.weight": (32,), "bn1.bias": (32,), "bn1.running_mean": (32,), "bn1.running_var": (32,), "bn1.num_batches_tracked": (),
          "fc.weight": (20, 576), "fc.bias": (20,),
          "bn2.weight": (20,), "bn2.bias": (20,), "bn2.running_mean": (20,), "bn2.running_var": (20,), "bn2.num_batches_tracked": ()}
RTOL = 1e-10


def fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)))
    z["ls"] = None if z["label_smoothing"] < 0 else float(z["label_smoothing"])
    z["rates"] = tuple(float(p) for p in z["dropouts"])
    z["masked"] = "mask_seed" in z
    return z


def tables(z):
    """The restatement's view of a fixture's state before the step."""
    P = {k: z[k].astype(np.float64) for k in TENSORS + BUFFERS}
    P["hidden_size_1"] = int(z["hidden_size_1"])
    return P


def recorded_masks(z):
    return [tuple(z["mask.%s.%d" % (d, s)] for s in range(3)) for d in ("tail", "head")] if z["masked"] else None


def state_dict_of(z):
    return {k: torch.from_numpy(np.asarray(z[k])) for k in SHAPES}


def build(**over):
    from pykg2vec_amd.projection import ConvE
    kw = dict(PARAMS)
    kw.update(over)
    return ConvE(**kw)


def close(got, want, scale=None):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() <= RTOL * max(np.abs(want).max(), scale or 0.0)


# ---------------------------------------------------------------- the restatement against the live reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_float64(name):
    z = fixture(name)
    P = tables(z)
    out = cr.step(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"], mask_list=recorded_masks(z))
    assert abs(out["loss"] - z["loss"]) <= RTOL * abs(z["loss"])
    assert close(out["pred_tails"], z["pred_tails"]) and close(out["pred_heads"], z["pred_heads"])
    for k in TENSORS:
        # the four gradients a training-mode batch norm cancels are rounding noise on both sides: compared on their cancellation scale
        assert close(out["grads"][k], z["grad." + k], out["scale"].get(k)), k
    for k in BUFFERS:
        assert close(out["buffers"][k], z["after." + k]), k
        assert not np.array_equal(z["after." + k], z[k]), k     # the step moved every running buffer
    for k in COUNTERS:
        assert int(z["after." + k]) == int(z[k]) + 2 and int(z[k]) == 2
    assert out["margin"] > 1e-5
    assert close(cr.forward(P, z["h"], z["r"], "tail"), z["eval_pred_tails"]) and close(cr.forward(P, z["t"], z["r"], "head"), z["eval_pred_heads"])
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    ranks, gap = cr.ranks(P, z["test"], known)
    assert np.array_equal(ranks, z["ranks"]) and gap > 1e-6


def test_without_dropout_four_gradients_vanish():
    z = fixture("conve")
    for k in cr.VANISHING:
        assert np.abs(z["grad." + k]).max() < 1e-5 * np.abs(z["grad.conv2d_1.weight"]).max(), k    # (bn0.weight survives through eps)


def test_restatement_masks_are_the_recorded_masks():
    z = fixture("conve_masked")
    B, k = len(z["h"]), int(z["hidden_size"])
    for side, want in enumerate(recorded_masks(z)):
        got = cr.masks(B, k, z["rates"], int(z["mask_seed"]), int(z["mask_offset"]), row0=side * B)
        for site in range(3):
            assert np.array_equal(got[site], want[site]), (side, site)
            p = np.float32(z["rates"][site])
            assert set(np.unique(want[site])) == {0.0, float(np.float32(1) / (np.float32(1) - p))}
    assert [m.shape for m in recorded_masks(z)[0]] == [(B, 2 * k), (B, 32), (B, k)]
    # the head direction's rows follow the tail direction's: another slice of the same draw, not the same masks
    assert not np.array_equal(z["mask.tail.0"], z["mask.head.0"])
    assert np.array_equal(cr.masks(2 * B, k, z["rates"], int(z["mask_seed"]), int(z["mask_offset"]))[1][B:], z["mask.head.1"])


def test_eval_form_skips_bn2_and_training_form_needs_two_rows():
    z = fixture("conve")
    P = tables(z)
    x, s, _ = cr.body(P, z["h"], z["r"], 0, train=False)
    assert np.array_equal(x, np.maximum(s["u"], 0))
    with pytest.raises(ValueError, match="more than 1 value"):
        cr.body(P, z["h"][:1], z["r"][:1], 0, train=True)


# ---------------------------------------------------------------- the drop-in class
@pytest.mark.parametrize("missing", sorted(PARAMS))
def test_constructor_names_the_missing_parameter(missing):
    from pykg2vec_amd.projection import ConvE
    kw = {k: v for k, v in PARAMS.items() if k != missing}
    with pytest.raises(Exception, match="hyperparameter %s not found" % missing):
        ConvE(**kw)


def test_class_contract_and_state_dict():
    from pykg2vec_amd import TrainingStrategy, import_model
    from pykg2vec_amd.criterion import Criterion
    from pykg2vec_amd.kgmeta import ProjectionModel
    m = build()
    assert import_model("conve") is type(m) and isinstance(m, ProjectionModel)
    assert m.model_name == "conve" and m.training_strategy == TrainingStrategy.PROJECTION_BASED
    assert m.loss is Criterion.multi_class_bce and m.get_reg(None, None, None) == 0 and m.lmbda == 0.1
    assert m.parameter_list == [m.ent_embeddings, m.rel_embeddings, m.b]
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES
    assert len(list(m.parameters())) == 13
    z = fixture("conve")
    assert {k: np.asarray(z[k]).shape for k in SHAPES} == SHAPES            # the live reference's state dict: the same keys and shapes
    m.load_state_dict(state_dict_of(z), strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), z[k]), k
    assert int(m.bn1.num_batches_tracked) == 2
    tt = m.trainable_tensors()
    named = dict(m.named_parameters())
    assert len(tt) == 13 and all(t is named[k] for t, k in zip(tt, TENSORS))
    assert [tuple(b.shape) for b in m.running_buffers()] == [SHAPES[k] for k in BUFFERS]
    with pytest.raises(AssertionError, match="Unknown forward direction"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), direction="sideways")
    e1, r1, e2 = m.embed(torch.tensor([1]), torch.tensor([7]), torch.tensor([2]))
    assert e1.shape == r1.shape == e2.shape == (1, 20) and torch.equal(m.embed2(torch.tensor([1]), torch.tensor([7]))[1], r1)


def test_default_init_is_the_reference_s():
    """nn.Embedding's N(0, 1) for the three tables (no xavier), torch's defaults for the layers."""
    torch.manual_seed(0)
    m = build(tot_entity=4000)
    assert abs(float(m.ent_embeddings.weight.std()) - 1.0) < 0.05
    assert float(m.bn1.weight.min()) == 1.0 and float(m.bn1.running_var.min()) == 1.0 and m.bn0.momentum == 0.1 and m.bn2.eps == 1e-5


# ---------------------------------------------------------------- C ABI
def test_struct_layout_agrees_with_header():
    from pykg2vec_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    body = re.search(r"typedef struct kge_conve_desc \{(.*?)\} kge_conve_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", x).strip(" *") for x in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [f[0] for f in _lib.ConveDesc._fields_]
    # 2 x int64, 2 x int32, 3 x float, int32, 2 x uint64, 6 x float, 32 pointers: no padding
    assert ctypes.sizeof(_lib.ConveDesc) == 16 + 8 + 12 + 4 + 16 + 24 + 32 * 8
    assert _lib.ConveDesc.seed.offset == 40 and _lib.ConveDesc.eps.offset == 56 and _lib.ConveDesc.ent.offset == 80
    assert _lib.ConveDesc.bn0_mean.offset == 80 + 13 * 8 and _lib.ConveDesc.g_ent.offset == 80 + 19 * 8
    assert re.search(r"#define KGE_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3      # untouched
    assert re.search(r"#define KGE_CONVE_MAX_HIDDEN %d\b" % _lib.CONVE_MAX_HIDDEN, header)


SYMBOLS = ["kge_conve_saved_floats", "kge_conve_body_forward", "kge_conve_body_backward", "kge_conve_train_bce", "kge_conve_eval_ranks"] + \
          ["kge_conve_%s_workspace_bytes" % s for s in ("body_forward", "body_backward", "train_bce", "eval_ranks")]


def test_symbols_are_exported():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


def _desc():
    from pykg2vec_amd import _lib
    d = _lib.ConveDesc()
    d.tot_entity, d.tot_relation, d.hidden_size, d.hidden_size_1, d.train = 10, 3, 20, 5, 1
    for i in range(3):
        d.eps[i], d.momentum[i] = 1e-5, 0.1
    for f in _lib.CONVE_TABLES + _lib.CONVE_BUFFERS + tuple("g_" + n for n in _lib.CONVE_TABLES):
        setattr(d, f, 0x1000)    # never dereferenced: every call below is refused before a launch
    return d


def _set(d, field, value):
    if isinstance(field, tuple):
        getattr(d, field[0])[field[1]] = value
    else:
        setattr(d, field, value)


@pytest.mark.parametrize("field,value,msg", [
    ("ent", None, "null tables"), ("bn2_var", None, "null tables"), ("hidden_size", 0, "must be positive"),
    ("hidden_size", 22, "hidden_size = 22 is no multiple of hidden_size_1 = 5"), ("hidden_size_1", 2, "smaller than the 3 x 3 filter"),
    ("hidden_size_1", 20, "smaller than the 3 x 3 filter"), ("hidden_size", 2000, "hidden_size = 2000 exceeds 1024"),
    (("momentum", 1), 0.0, "momentum 1 must be in (0, 1]"), (("momentum", 2), 1.5, "momentum 2 must be in (0, 1]"),
    ("feature_map_dropout", 1.0, "dropout rate 1"), ("input_dropout", -0.1, "dropout rate 0"), ("offset", 1 << 62, "offset"),
    ("g_fc_w", None, "null gradient buffers")])
def test_entry_points_refuse_bad_descriptors(field, value, msg):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    _set(d, field, value)
    p = ctypes.c_void_p(0x1000)
    rc = lib.kge_conve_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, 1 << 40, p, None)
    assert rc != 0 and msg in lib.kge_last_error().decode() and "kge_conve_train_bce" in lib.kge_last_error().decode()
    if field != "g_fc_w":
        assert lib.kge_conve_body_forward_workspace_bytes(ctypes.byref(d), 4) == 0
        assert lib.kge_conve_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, 1 << 40, p, None, None) != 0
        assert "kge_conve_eval_ranks" in lib.kge_last_error().decode()


def test_entry_points_refuse_one_training_row_small_workspaces_and_eval_backward():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    p = ctypes.c_void_p(0x1000)
    big = 1 << 40
    assert lib.kge_conve_body_forward(ctypes.byref(d), p, p, 1, 0, 0, p, p, p, big, None) != 0
    assert "kge_conve_body_forward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_conve_train_bce(ctypes.byref(d), p, p, p, 1, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "needs more than one row" in lib.kge_last_error().decode()
    need = lib.kge_conve_body_forward_workspace_bytes(ctypes.byref(d), 4)
    assert need > 0
    assert lib.kge_conve_body_forward(ctypes.byref(d), p, p, 4, 0, 0, p, p, p, need - 1, None) != 0
    assert "kge_conve_body_forward: workspace too small" in lib.kge_last_error().decode()
    assert lib.kge_conve_body_forward(ctypes.byref(d), p, p, 4, 2, 0, p, p, p, need, None) != 0 and "side must be 0 or 1" in lib.kge_last_error().decode()
    assert lib.kge_conve_body_backward(ctypes.byref(d), p, p, 4, 0, 0, p, p, None, 0, None) != 0
    need = lib.kge_conve_train_bce_workspace_bytes(ctypes.byref(d), 4, 1, 1)
    assert lib.kge_conve_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, need - 1, p, None) != 0
    assert "kge_conve_train_bce: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_conve_eval_ranks_workspace_bytes(ctypes.byref(d), 4)
    assert lib.kge_conve_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, need - 1, p, None, None) != 0
    assert "kge_conve_eval_ranks: workspace too small" in lib.kge_last_error().decode()
    d.train = 0
    assert lib.kge_conve_body_forward_workspace_bytes(ctypes.byref(d), 1) > 0      # one row is fine in the eval form
    assert lib.kge_conve_body_backward(ctypes.byref(d), p, p, 4, 0, 0, p, p, p, big, None) != 0
    assert "the eval form (train = 0) has no backward" in lib.kge_last_error().decode()
