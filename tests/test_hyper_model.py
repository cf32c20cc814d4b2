"""HypER without a GPU: the float64 restatement (tools/hyper_reference.py) reproduces the live reference's float64 outputs frozen in
tests/golden/ref_hyper{,_ls,_masked}.npz (1e-10, ranks exact), the recorded Philox masks and the padding rows (padding_idx = 0 on both
embeddings); the drop-in class keeps the reference's construction contract and state dict; every refusal that needs no device raises
with its sentence; the ctypes struct agrees with the header."""
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
from tools import hyper_reference as hr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["hyper", "hyper_ls", "hyper_masked"]
TENSORS, BUFFERS, COUNTERS = hr.TENSORS, hr.BUFFERS, hr.COUNTERS
PARAMS = dict(tot_entity=70, tot_relation=5, ent_hidden_size=20, rel_hidden_size=12, input_dropout=0.2, hidden_dropout=0.3,
              feature_map_dropout=0.2)
# the reference's state dict, in its order: the bare parameter b first, then the modules in registration order
SHAPES = [("b", (70,)), ("ent_embeddings.weight", (70, 20)), ("rel_embeddings.weight", (5, 12)),
          ("bn0.weight", (1,)), ("bn0.bias", (1,)), ("bn0.running_mean", (1,)), ("bn0.running_var", (1,)), ("bn0.num_batches_tracked", ()),
          ("bn1.weight", (32,)), ("bn1.bias", (32,)), ("bn1.running_mean", (32,)), ("bn1.running_var", (32,)), ("bn1.num_batches_tracked", ()),
          ("bn2.weight", (20,)), ("bn2.bias", (20,)), ("bn2.running_mean", (20,)), ("bn2.running_var", (20,)), ("bn2.num_batches_tracked", ()),
          ("fc.weight", (20, 384)), ("fc.bias", (20,)), ("fc1.weight", (288, 12)), ("fc1.bias", (288,))]
RTOL = 1e-10


def fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)))
    z["ls"] = None if z["label_smoothing"] < 0 else float(z["label_smoothing"])
    z["rates"] = tuple(float(p) for p in z["dropouts"])
    z["masked"] = "mask_seed" in z
    return z


def tables(z):
    """The restatement's view of a fixture's state before the step."""
    return {k: z[k].astype(np.float64) for k in TENSORS + BUFFERS}


def recorded_masks(z):
    return [tuple(z["mask.%s.%d" % (d, s)] for s in range(3)) for d in ("tail", "head")] if z["masked"] else None


def state_dict_of(z):
    return {k: torch.from_numpy(np.asarray(z[k])) for k, _ in SHAPES}


def build(**over):
    from pykg2vec_amd.projection import HypER
    kw = dict(PARAMS)
    kw.update(over)
    return HypER(**kw)


def close(got, want, scale=None):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() <= RTOL * max(np.abs(want).max(), scale or 0.0)


# ---------------------------------------------------------------- the restatement against the live reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_float64(name):
    z = fixture(name)
    P = tables(z)
    out = hr.step(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"], mask_list=recorded_masks(z))
    assert abs(out["loss"] - z["loss"]) <= RTOL * abs(z["loss"])
    assert close(out["pred_tails"], z["pred_tails"]) and close(out["pred_heads"], z["pred_heads"])
    vanishing = hr.VANISHING(z["rates"], P["bn0.bias"])
    for k in TENSORS:
        # a gradient that vanishes analytically is rounding noise on both sides: compared on its cancellation scale
        assert close(out["grads"][k], z["grad." + k], out["scale"][k] if k in vanishing else None), k
    for k in BUFFERS:
        assert close(out["buffers"][k], z["after." + k]), k
        assert not np.array_equal(z["after." + k], z[k]), k     # the step moved every running buffer
    for k in COUNTERS:
        assert int(z["after." + k]) == int(z[k]) + 2 and int(z[k]) == 2
    assert out["margin"] > 1e-5 and hr.eval_margin(P, z["test"]) > 1e-5
    assert close(hr.forward(P, z["h"], z["r"], "tail"), z["eval_pred_tails"]) and close(hr.forward(P, z["t"], z["r"], "head"), z["eval_pred_heads"])
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    ranks, gap = hr.ranks(P, z["test"], known)
    assert np.array_equal(ranks, z["ranks"]) and gap > 1e-6


def test_vanishing_rule_follows_the_rates():
    assert hr.VANISHING((0.0, 0.0, 0.0)) == ("bn0.weight", "fc.bias", "bn1.bias")
    assert hr.VANISHING((0.0, 0.2, 0.0)) == ("bn0.weight", "fc.bias")
    assert hr.VANISHING((0.2, 0.2, 0.3)) == ("bn0.weight",)
    assert hr.VANISHING((0.2, 0.2, 0.3), np.array([0.25])) == ()      # bn0.bias != 0: bn0.weight no longer only scales the conv output
    z = fixture("hyper")
    big = np.abs(z["grad.bn1.weight"]).max()
    for k in ("fc.bias", "bn1.bias"):
        assert np.abs(z["grad." + k]).max() < 1e-9 * big, k
    for k in ("bn0.bias", "fc1.bias"):     # the per-row filter keeps bn1 from cancelling these
        assert np.abs(z["grad." + k]).max() > 1e-4 * big, k
    z = fixture("hyper_masked")
    assert np.abs(z["grad.fc.bias"]).max() > 1e-4 * big and np.abs(z["grad.bn1.bias"]).max() > 1e-4 * big


def test_bn0_weight_survives_only_through_eps_at_default_init():
    """Quirk 5: with bn0.bias = 0 the gradient of bn0.weight is orders of magnitude below its neighbours'."""
    z = fixture("hyper")
    P = tables(z)
    P["bn0.bias"] = np.zeros(1)
    P["bn0.weight"] = np.ones(1)
    out = hr.step(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"])
    assert abs(out["grads"]["bn0.weight"][0]) < 1e-3 * abs(out["grads"]["bn0.bias"][0])
    assert abs(out["grads"]["bn0.weight"][0]) < 1e-6 * out["scale"]["bn0.weight"]


def test_restatement_masks_are_the_recorded_masks():
    z = fixture("hyper_masked")
    B, D = len(z["h"]), int(z["ent_hidden_size"])
    for side, want in enumerate(recorded_masks(z)):
        got = hr.masks(B, D, z["rates"], int(z["mask_seed"]), int(z["mask_offset"]), row0=side * B)
        for site in range(3):
            assert np.array_equal(got[site], want[site]), (side, site)
            p = np.float32(z["rates"][site])
            assert set(np.unique(want[site])) == {0.0, float(np.float32(1) / (np.float32(1) - p))}
    assert [m.shape for m in recorded_masks(z)[0]] == [(B, D), (B, 32), (B, D)]
    # the head direction's rows follow the tail direction's: another slice of the same draw, not the same masks
    assert not np.array_equal(z["mask.tail.0"], z["mask.head.0"])
    assert np.array_equal(hr.masks(2 * B, D, z["rates"], int(z["mask_seed"]), int(z["mask_offset"]))[1][B:], z["mask.head.1"])


@pytest.mark.parametrize("name", NAMES)
def test_padding_rows(name):
    """padding_idx = 0 on both embeddings: the lookup's gradient of id 0 is dropped; row 0 itself is an ordinary row."""
    z = fixture(name)
    assert (z["h"] == 0).sum() == 1 and (z["t"] == 0).sum() == 1 and (z["r"] == 0).any() and (z["test"] == 0).any()
    assert np.abs(z["ent_embeddings.weight"][0]).min() > 0 and np.abs(z["rel_embeddings.weight"][0]).min() > 0
    assert np.array_equal(z["grad.rel_embeddings.weight"][0], np.zeros(12))
    out = hr.step(tables(z), z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"], mask_list=recorded_masks(z))
    assert np.array_equal(out["grads"]["rel_embeddings.weight"][0], np.zeros(12))
    assert close(out["head_ent0"], z["grad.ent_embeddings.weight"][0]) and np.abs(out["head_ent0"]).max() > 0
    # a non-zero id of the batch receives the body's share too
    e1, r1 = int(z["h"][z["h"] != 0][0]), int(z["r"][z["r"] != 0][0])
    assert np.abs(z["grad.rel_embeddings.weight"][r1]).max() > 0
    body_share = out["grads"]["ent_embeddings.weight"][e1] - _head_share(z, out, e1)
    assert np.abs(body_share).max() > 1e-3 * np.abs(out["grads"]["ent_embeddings.weight"][e1]).max()
    assert close(_head_share(z, out, 0), out["head_ent0"])


def _head_share(z, out, row):
    """The head's share dlogit^T x of grad(ent)[row], from the restatement's predictions."""
    P = tables(z)
    E = int(z["E"])
    B = len(z["h"])
    total = np.zeros(P["ent_embeddings.weight"].shape[1])
    masks = recorded_masks(z)
    for side, (ee, yy, p) in enumerate(((z["h"], z["hr_t"], out["pred_tails"]), (z["t"], z["tr_h"], out["pred_heads"]))):
        x, _, _ = hr.body(P, ee, z["r"], masks[side] if masks else None, True)
        Y = yy if z["ls"] is None else yy * (1.0 - z["ls"]) + 1.0 / E
        dlogit = (hr.sigmoid(p) - Y) / (B * E) * p * (1 - p)
        total += dlogit[:, row] @ x
    return total


def test_eval_form_applies_bn2_with_the_running_buffers_and_training_form_needs_two_rows():
    z = fixture("hyper")
    P = tables(z)
    x, s, stats = hr.body(P, z["h"], z["r"], train=False)
    want = (s["u"] - P["bn2.running_mean"]) / np.sqrt(P["bn2.running_var"] + 1e-5) * P["bn2.weight"] + P["bn2.bias"]
    assert np.array_equal(x, np.maximum(want, 0)) and not np.array_equal(x, np.maximum(s["u"], 0)) and stats == {}
    P2 = dict(P)
    P2["bn2.running_mean"] = P["bn2.running_mean"] + 0.5
    assert not np.array_equal(hr.body(P2, z["h"], z["r"], train=False)[0], x)
    with pytest.raises(ValueError, match="more than 1 value"):
        hr.body(P, z["h"][:1], z["r"][:1], train=True)
    # one relation table: the direction selects nothing
    assert np.array_equal(hr.forward(P, z["h"], z["r"], "tail"), hr.forward(P, z["h"], z["r"], "head"))


# ---------------------------------------------------------------- the drop-in class
@pytest.mark.parametrize("missing", sorted(PARAMS))
def test_constructor_names_the_missing_parameter(missing):
    from pykg2vec_amd.projection import HypER
    kw = {k: v for k, v in PARAMS.items() if k != missing}
    with pytest.raises(Exception, match="hyperparameter %s not found" % missing):
        HypER(**kw)


def test_class_contract_and_state_dict():
    from pykg2vec_amd import TrainingStrategy, import_model
    from pykg2vec_amd.criterion import Criterion
    from pykg2vec_amd.kgmeta import ProjectionModel
    m = build(device="cpu")
    assert import_model("hyper") is type(m) and isinstance(m, ProjectionModel) and m.kernel_name == "hyper" and m.device == "cpu"
    assert build().device == torch.device("cpu")
    assert m.model_name == "hyper" and m.training_strategy == TrainingStrategy.PROJECTION_BASED
    assert m.loss is Criterion.multi_class_bce and m.get_reg(None, None, None) == 0
    assert m.parameter_list == [m.ent_embeddings, m.rel_embeddings]
    assert m.ent_embeddings.padding_idx == 0 and m.rel_embeddings.padding_idx == 0
    assert m.ent_embeddings.name == "ent_embeddings" and m.rel_embeddings.name == "rel_embeddings"
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == SHAPES          # keys, ORDER and shapes
    assert len(list(m.parameters())) == 13
    z = fixture("hyper")
    assert [str(k) for k in z["state_keys"]] == [k for k, _ in SHAPES]      # the live reference's state dict: the same keys in the same order
    assert [np.asarray(z[k]).shape for k, _ in SHAPES] == [s for _, s in SHAPES]
    m.load_state_dict(state_dict_of(z), strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), z[k]), k
    assert int(m.bn1.num_batches_tracked) == 2
    tt = m.trainable_tensors()
    named = dict(m.named_parameters())
    assert list(named) == list(TENSORS)
    assert len(tt) == 13 and all(t is named[k] for t, k in zip(tt, TENSORS)) and tt[0] is m.b
    assert [tuple(b.shape) for b in m.running_buffers()] == [dict(SHAPES)[k] for k in BUFFERS]
    with pytest.raises(AssertionError, match="Unknown forward direction"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), direction="sideways")
    e1, r1, e2 = m.embed(torch.tensor([1]), torch.tensor([4]), torch.tensor([2]))
    assert e1.shape == e2.shape == (1, 20) and r1.shape == (1, 12) and torch.equal(m.embed2(torch.tensor([1]), torch.tensor([4]))[1], r1)


def test_default_init_is_the_reference_s():
    """xavier_uniform_ on both tables AFTER padding_idx zeroed row 0 (so row 0 is an ordinary row), b zero, torch's defaults elsewhere."""
    torch.manual_seed(0)
    m = build(tot_entity=4000)
    for w in (m.ent_embeddings.weight.detach(), m.rel_embeddings.weight.detach()):
        bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
        assert float(w[0].abs().min()) > 0
    assert m.b.shape == (4000,) and float(m.b.abs().max()) == 0.0 and isinstance(m.b, torch.nn.Parameter)
    assert float(m.bn1.weight.min()) == 1.0 and float(m.bn1.running_var.min()) == 1.0 and m.bn0.momentum == 0.1 and m.bn2.eps == 1e-5


def test_cpu_tensors_are_refused():
    m = build()
    with pytest.raises(Exception, match="kge::hyper_body: ids and tables must live on the HIP device"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))


# ---------------------------------------------------------------- C ABI
def test_struct_layout_agrees_with_header():
    from pykg2vec_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    body = re.search(r"typedef struct kge_hyper_desc \{(.*?)\} kge_hyper_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", x).strip(" *") for x in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [f[0] for f in _lib.HyperDesc._fields_]
    assert names[12:25] == list(_lib.HYPER_TABLES) and names[12] == "b"           # state-dict order: b first
    # 2 x int64, 2 x int32, 3 x float, int32, 2 x uint64, 6 x float, 32 pointers: no padding
    assert ctypes.sizeof(_lib.HyperDesc) == 16 + 8 + 12 + 4 + 16 + 24 + 32 * 8
    assert _lib.HyperDesc.seed.offset == 40 and _lib.HyperDesc.eps.offset == 56 and _lib.HyperDesc.b.offset == 80
    assert _lib.HyperDesc.bn0_mean.offset == 80 + 13 * 8 and _lib.HyperDesc.g_b.offset == 80 + 19 * 8
    assert re.search(r"#define KGE_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3      # untouched
    assert re.search(r"#define KGE_HYPER_MAX_HIDDEN %d\b" % _lib.HYPER_MAX_HIDDEN, header) and _lib.HYPER_MAX_HIDDEN >= 256


SYMBOLS = ["kge_hyper_saved_floats", "kge_hyper_body_forward", "kge_hyper_body_backward", "kge_hyper_train_bce", "kge_hyper_eval_ranks"] + \
          ["kge_hyper_%s_workspace_bytes" % s for s in ("body_forward", "body_backward", "train_bce", "eval_ranks")]


def test_symbols_are_exported():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


def _desc():
    from pykg2vec_amd import _lib
    d = _lib.HyperDesc()
    d.tot_entity, d.tot_relation, d.ent_hidden_size, d.rel_hidden_size, d.train = 10, 3, 20, 12, 1
    for i in range(3):
        d.eps[i], d.momentum[i] = 1e-5, 0.1
    for f in _lib.HYPER_TABLES + _lib.HYPER_BUFFERS + tuple("g_" + n for n in _lib.HYPER_TABLES):
        setattr(d, f, 0x1000)    # never dereferenced: every call below is refused before a launch
    return d


def _set(d, field, value):
    if isinstance(field, tuple):
        getattr(d, field[0])[field[1]] = value
    else:
        setattr(d, field, value)


@pytest.mark.parametrize("field,value,msg", [
    ("ent", None, "null tables"), ("b", None, "null tables"), ("fc1_w", None, "null tables"), ("bn2_var", None, "null tables"),
    ("ent_hidden_size", 0, "must be positive"), ("rel_hidden_size", 0, "must be positive"),
    ("ent_hidden_size", 8, "ent_hidden_size = 8 is shorter than the 9-tap filter"),
    ("ent_hidden_size", 2000, "ent_hidden_size = 2000 / rel_hidden_size = 12 exceeds 1024"),
    ("rel_hidden_size", 1025, "ent_hidden_size = 20 / rel_hidden_size = 1025 exceeds 1024"),
    (("momentum", 1), 0.0, "momentum 1 must be in (0, 1]"), (("momentum", 2), 1.5, "momentum 2 must be in (0, 1]"),
    (("eps", 0), -1.0, "eps 0 must not be negative"),
    ("feature_map_dropout", 1.0, "dropout rate 1"), ("input_dropout", -0.1, "dropout rate 0"), ("offset", 1 << 62, "offset"),
    ("g_fc1_w", None, "null gradient buffers")])
def test_entry_points_refuse_bad_descriptors(field, value, msg):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    _set(d, field, value)
    p = ctypes.c_void_p(0x1000)
    rc = lib.kge_hyper_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, 1 << 40, p, None)
    assert rc != 0 and msg in lib.kge_last_error().decode() and "kge_hyper_train_bce" in lib.kge_last_error().decode()
    if field != "g_fc1_w":
        assert lib.kge_hyper_body_forward_workspace_bytes(ctypes.byref(d), 4) == 0
        assert lib.kge_hyper_saved_floats(ctypes.byref(d), 4) == 0
        assert lib.kge_hyper_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, 1 << 40, p, None, None) != 0
        assert "kge_hyper_eval_ranks" in lib.kge_last_error().decode()
        assert lib.kge_hyper_body_forward(ctypes.byref(d), p, p, 4, 0, p, p, p, 1 << 40, None) != 0
        assert "kge_hyper_body_forward" in lib.kge_last_error().decode()
    assert lib.kge_hyper_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, p, 1 << 40, None) != 0
    assert "kge_hyper_body_backward" in lib.kge_last_error().decode()


def test_smallest_and_largest_sizes_are_accepted():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    d.ent_hidden_size, d.rel_hidden_size = 9, 1
    assert lib.kge_hyper_saved_floats(ctypes.byref(d), 4) == 4 * (32 + 9 + 288) + 66 + 18
    d.ent_hidden_size, d.rel_hidden_size = 1024, 1024
    assert lib.kge_hyper_body_forward_workspace_bytes(ctypes.byref(d), 4) > 0


def test_entry_points_refuse_one_training_row_small_workspaces_and_eval_backward():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    p = ctypes.c_void_p(0x1000)
    big = 1 << 40
    assert lib.kge_hyper_body_forward(ctypes.byref(d), p, p, 1, 0, p, p, p, big, None) != 0
    assert "kge_hyper_body_forward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_hyper_body_backward(ctypes.byref(d), p, p, 1, 0, p, p, p, big, None) != 0
    assert "kge_hyper_body_backward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_hyper_train_bce(ctypes.byref(d), p, p, p, 1, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "kge_hyper_train_bce" in lib.kge_last_error().decode() and "needs more than one row" in lib.kge_last_error().decode()
    need = lib.kge_hyper_body_forward_workspace_bytes(ctypes.byref(d), 4)
    assert need > 0
    assert lib.kge_hyper_body_forward(ctypes.byref(d), p, p, 4, 0, p, p, p, need - 1, None) != 0
    assert "kge_hyper_body_forward: workspace too small" in lib.kge_last_error().decode()
    assert lib.kge_hyper_body_forward(ctypes.byref(d), p, p, 4, -1, p, p, p, need, None) != 0 and "row0 + n below 2^32" in lib.kge_last_error().decode()
    assert lib.kge_hyper_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, None, 0, None) != 0
    assert "kge_hyper_body_backward: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_hyper_train_bce_workspace_bytes(ctypes.byref(d), 4, 1, 1)
    assert lib.kge_hyper_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, need - 1, p, None) != 0
    assert "kge_hyper_train_bce: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_hyper_eval_ranks_workspace_bytes(ctypes.byref(d), 4)
    assert lib.kge_hyper_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, need - 1, p, None, None) != 0
    assert "kge_hyper_eval_ranks: workspace too small" in lib.kge_last_error().decode()
    d.train = 0
    assert lib.kge_hyper_body_forward_workspace_bytes(ctypes.byref(d), 1) > 0      # one row is fine in the eval form
    assert lib.kge_hyper_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, p, big, None) != 0
    assert "kge_hyper_body_backward: the eval form (train = 0) has no backward" in lib.kge_last_error().decode()
    assert lib.kge_hyper_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "kge_hyper_train_bce: the step is the training form" in lib.kge_last_error().decode()
