"""AcrE without a GPU: the float64 restatement (tools/acre_reference.py) reproduces the live reference's float64 outputs frozen in
tests/golden/ref_acre{,_ls,_masked,_parallel,_parallel_masked}.npz (1e-10, ranks exact; the two large gradients at the recorded sample)
and the recorded Philox masks; the drop-in class keeps the reference's construction contract and state dict in both ways and with
both acre_bias values; every refusal that needs no device raises with its sentence; the ctypes struct agrees with the header."""
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
from tools import acre_reference as ar  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SERIAL = ["acre", "acre_ls", "acre_masked"]
NAMES = SERIAL + ["acre_parallel", "acre_parallel_masked"]
BUFFERS, COUNTERS = ar.BUFFERS, ar.COUNTERS
PARAMS = dict(tot_entity=70, tot_relation=5, hidden_size=200, input_dropout=0.2, hidden_dropout=0.3, feature_map_dropout=0.2,
              in_channels=3, way="serial", first_atrous=1, second_atrous=2, third_atrous=3, acre_bias=True)
RTOL = 1e-10


def fixture(name):
    z, G, P = ar.load_fixture(os.path.join(GOLDEN, "ref_%s.npz" % name))
    z["ls"] = None if z["label_smoothing"] < 0 else float(z["label_smoothing"])
    z["rates"] = tuple(float(p) for p in z["dropouts"])
    z["masked"] = "mask_seed" in z
    z["G"], z["P"], z["TENSORS"] = G, P, ar.tensors(G)
    return z


def tables(z):
    """The restatement's view of a fixture's state before the step (the large tensors regenerated from their recorded seeds)."""
    return dict(z["P"])


def recorded_masks(z):
    return [tuple(z["mask.%s.%d" % (d, s)] for s in range(3)) for d in ("tail", "head")] if z["masked"] else None


def recorded_grad_error(z, key, got):
    """(largest error of `got` against the recorded gradient, its max-abs): the large gradients at their recorded sample and sum."""
    got = np.asarray(got, dtype=np.float64)
    if key in ar.LARGE:
        idx = z["grad_index." + key]
        assert np.array_equal(idx[:-1], ar.sample_index(int(z["grad_sample_seed." + key]), got.size))
        return np.abs(got.reshape(-1)[idx] - z["grad_sample." + key]).max(), float(z["grad_maxabs." + key])
    return np.abs(got - z["grad." + key]).max(), np.abs(z["grad." + key]).max()


def state_dict_of(z):
    return {str(k): torch.from_numpy(np.asarray(z[str(k)])) for k in z["state_keys"]}


def build(**over):
    from pykg2vec_amd.projection import AcrE
    kw = dict(PARAMS)
    kw.update(over)
    return AcrE(**kw)


def close(got, want, scale=None):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() <= RTOL * max(np.abs(want).max(), scale or 0.0)


# ---------------------------------------------------------------- the restatement against the live reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_float64(name):
    z = fixture(name)
    P, G = tables(z), z["G"]
    out = ar.step(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"], mask_list=recorded_masks(z))
    assert abs(out["loss"] - z["loss"]) <= RTOL * abs(z["loss"])
    assert close(out["pred_tails"], z["pred_tails"]) and close(out["pred_heads"], z["pred_heads"])
    vanishing = ar.vanishing(G, z["rates"], P)
    for k in z["TENSORS"]:
        err, size = recorded_grad_error(z, k, out["grads"][k])
        # a gradient that vanishes analytically is rounding noise on both sides: compared on its cancellation scale
        assert err <= RTOL * max(size, out["scale"][k] if k in vanishing else 0.0), k
        if k in ar.LARGE:
            assert abs(np.abs(out["grads"][k]).max() - z["grad_maxabs." + k]) <= RTOL * z["grad_maxabs." + k]
            assert abs(out["grads"][k].sum() - z["grad_sum." + k]) <= 1e-9 * np.abs(out["grads"][k]).sum()
    for k in BUFFERS:
        assert close(out["buffers"][k], z["after." + k]), k
        assert not np.array_equal(z["after." + k], z[k]), k     # the step moved every running buffer
    for k in COUNTERS:
        assert int(z["after." + k]) == int(z[k]) + 2 and int(z[k]) == 2
    assert out["margin"] > 1e-5 and ar.eval_margin(P, G, z["test"]) > 1e-5     # bn1 and bn2 both feed a relu
    assert close(ar.forward(P, G, z["h"], z["r"], "tail"), z["eval_pred_tails"])
    assert close(ar.forward(P, G, z["t"], z["r"], "head"), z["eval_pred_heads"])
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    ranks, gap = ar.ranks(P, G, z["test"], known)
    assert np.array_equal(ranks, z["ranks"]) and gap > 1e-6
    # no padding_idx: id 0 of both tables is in the batch and its lookup gradient is an ordinary row; rows R .. 2R-1 get nothing
    assert (z["h"] == 0).sum() == 1 and (z["t"] == 0).sum() == 1 and (z["r"] == 0).any() and (z["test"] == 0).any()
    assert np.abs(z["grad.rel_embeddings.weight"][0]).max() > 0 and not z["grad.rel_embeddings.weight"][5:].any()


def test_a_permuted_sum_order_is_the_same_model():
    z = fixture("acre_masked")
    kw = dict(label_smoothing=z["ls"], mask_list=recorded_masks(z))
    a = ar.step(tables(z), z["G"], z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **kw)
    b = ar.step(tables(z), z["G"], z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], order=5, **kw)
    assert abs(a["loss"] - b["loss"]) < 1e-13
    for k in z["TENSORS"]:
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= 1e-12 * max(np.abs(a["grads"][k]).max(), a["scale"].get(k, 0.0)), k


def test_vanishing_rule():
    z = fixture("acre")
    G = z["G"]
    assert ar.vanishing(G, (0.0, 0.0, 0.0)) == ("fc.bias", "conv3.bias")
    assert ar.vanishing(G, (0.2, 0.2, 0.3)) == ("conv3.bias",)
    assert ar.vanishing(dict(G, acre_bias=False), (0.2, 0.2, 0.3)) == ()
    assert ar.vanishing(dict(G, way="parallel"), (0.0, 0.0, 0.0)) == ("fc.bias",)
    big = np.abs(z["grad.bn1.weight"]).max()
    for k in ("fc.bias", "conv3.bias"):
        assert np.abs(z["grad." + k]).max() < 1e-9 * big, k
    for k in ("bn0.bias", "bn0.weight", "conv1.bias", "conv2.bias"):     # ZERO padding: the border keeps them alive
        assert np.abs(z["grad." + k]).max() > 1e-4 * big, k
    z = fixture("acre_masked")
    assert np.abs(z["grad.conv3.bias"]).max() < 1e-9 * big and np.abs(z["grad.fc.bias"]).max() > 1e-4 * big
    z = fixture("acre_parallel")
    for k in ("conv1.bias", "conv2.bias", "conv3.bias", "W_gate_e.bias", "bn0.bias"):
        assert np.abs(z["grad." + k]).max() > 1e-4 * np.abs(z["grad.bn1.weight"]).max(), k


def test_restatement_masks_are_the_recorded_masks():
    for name in ("acre_masked", "acre_parallel_masked"):
        z = fixture(name)
        B = len(z["h"])
        for side, want in enumerate(recorded_masks(z)):
            got = ar.masks(B, z["G"], z["rates"], int(z["mask_seed"]), int(z["mask_offset"]), row0=side * B)
            for site in range(3):
                assert np.array_equal(got[site], want[site]), (side, site)
                p = np.float32(z["rates"][site])
                assert set(np.unique(want[site])) == {0.0, float(np.float32(1) / (np.float32(1) - p))}
        assert [m.shape for m in recorded_masks(z)[0]] == [(B, 20, 20), (B, 3), (B, 200)]
        assert not np.array_equal(z["mask.tail.0"], z["mask.head.0"])


def test_dilated_convolution_against_a_direct_loop():
    """The restated convolution (zero padding = dilation) against explicit loops with bounds tests, and torch's own."""
    rng = np.random.default_rng(3)
    x, w, b = rng.normal(size=(2, 3, 20, 20)), rng.normal(size=(4, 3, 3, 3)), rng.normal(size=4)
    for d in (1, 3, 4):
        want = np.zeros((2, 4, 20, 20))
        for y in range(20):
            for xx in range(20):
                for i in range(3):
                    for j in range(3):
                        yy, xj = y + (i - 1) * d, xx + (j - 1) * d
                        if 0 <= yy < 20 and 0 <= xj < 20:
                            want[:, :, y, xx] += x[:, :, yy, xj] @ w[:, :, i, j].T
        want += b[None, :, None, None]
        got = ar.conv(x, w, b, d)
        assert np.abs(got - want).max() < 1e-12
        ref = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 1, d, d).numpy()
        assert np.abs(got - ref).max() < 1e-12


# ---------------------------------------------------------------- the drop-in class
@pytest.mark.parametrize("missing", sorted(PARAMS))
def test_constructor_names_the_missing_parameter(missing):
    from pykg2vec_amd.projection import AcrE
    kw = {k: v for k, v in PARAMS.items() if k != missing}
    with pytest.raises(Exception, match="hyperparameter %s not found" % missing):
        AcrE(**kw)


def test_class_contract():
    import pykg2vec_amd as pa
    from pykg2vec_amd import TrainingStrategy, import_model
    from pykg2vec_amd.criterion import Criterion
    from pykg2vec_amd.kgmeta import ProjectionModel
    m = build()
    assert pa.MODEL_MAP["acre"] == "projection.AcrE"
    assert import_model("acre") is type(m) and import_model("AcrE") is type(m) and isinstance(m, ProjectionModel) and m.kernel_name == "acre"
    assert m.model_name == "acre" and m.training_strategy == TrainingStrategy.PROJECTION_BASED
    assert m.loss is Criterion.multi_class_bce and m.get_reg(None, None, None) == 0
    assert m.parameter_list == [m.ent_embeddings, m.rel_embeddings]
    assert m.ent_embeddings.padding_idx is None and m.rel_embeddings.padding_idx is None
    assert tuple(m.rel_embeddings.weight.shape) == (10, 200)      # every relation and its reciprocal
    with pytest.raises(AssertionError, match="Unknown forward direction"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), direction="sideways")
    e1, r1, e2 = m.embed(torch.tensor([1]), torch.tensor([9]), torch.tensor([2]))
    assert e1.shape == e2.shape == r1.shape == (1, 200) and torch.equal(m.embed2(torch.tensor([1]), torch.tensor([9]))[1], r1)
    assert m.dropout_seed == 0 and m.dropout_offset == 0 and build(seed=7).dropout_seed == 7


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_is_the_reference_s(name):
    z = fixture(name)
    G = z["G"]
    m = build(way=G["way"], acre_bias=G["acre_bias"])
    keys = [str(k) for k in z["state_keys"]]
    sd = m.state_dict()
    assert list(sd) == keys and keys[0] == "bias"                          # keys and ORDER: the bare parameter first
    assert [tuple(v.shape) for v in sd.values()] == [np.asarray(z[k]).shape for k in keys]
    assert [k for k in keys if "running" not in k and "num_batches" not in k] == list(z["TENSORS"]) == [k for k, _ in m.named_parameters()]
    assert len(z["TENSORS"]) == {("serial", True): 17, ("serial", False): 14, ("parallel", True): 19}[(G["way"], G["acre_bias"])]
    m.load_state_dict(state_dict_of(z), strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), z[k]), k
    assert int(m.bn1.num_batches_tracked) == 2
    named = dict(m.named_parameters())
    tt = m.trainable_tensors()
    assert len(tt) == len(z["TENSORS"]) and all(t is named[k] for t, k in zip(tt, z["TENSORS"])) and tt[0] is m.bias
    shp = ar.shapes(G, 70, 5)
    assert [tuple(b.shape) for b in m.running_buffers()] == [shp[k] for k in BUFFERS]
    assert [tuple(t.shape) for t in tt] == [shp[k] for k in z["TENSORS"]]


def test_state_dict_of_the_parallel_way_without_bias():
    m = build(way="parallel", acre_bias=False)
    G = dict(in_channels=3, way="parallel", first_atrous=1, second_atrous=2, third_atrous=3, acre_bias=False)
    assert [k for k, _ in m.named_parameters()] == list(ar.tensors(G)) and len(ar.tensors(G)) == 16
    assert tuple(m.conv2.weight.shape) == (3, 1, 3, 3) and tuple(build().conv2.weight.shape) == (3, 3, 3, 3)


def test_default_init_is_the_reference_s():
    """xavier_uniform_ on both tables, bias zero, torch's defaults elsewhere; the gate only in the parallel way."""
    torch.manual_seed(0)
    m = build(tot_entity=4000, in_channels=32)
    for w in (m.ent_embeddings.weight.detach(), m.rel_embeddings.weight.detach()):
        bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
        assert float(w[0].abs().min()) > 0
    assert m.bias.shape == (4000,) and float(m.bias.detach().abs().max()) == 0.0 and isinstance(m.bias, torch.nn.Parameter)
    assert float(m.bn1.weight.min()) == 1.0 and float(m.bn1.running_var.min()) == 1.0 and m.bn0.momentum == 0.1 and m.bn2.eps == 1e-5
    assert m.bn0.num_features == 1 and m.bn1.num_features == 32 and m.fc.in_features == 400 * 32 and m.fc.out_features == 200
    assert m.conv3.dilation == (3, 3) and m.conv3.padding == (3, 3) and m.conv1.in_channels == 1 and m.conv2.in_channels == 32
    assert not hasattr(m, "W_gate_e")
    g = build(way="parallel").W_gate_e
    assert (g.in_features, g.out_features) == (1600, 400)


def test_cpu_tensors_are_refused():
    m = build()
    with pytest.raises(Exception, match="kge::acre_body: ids and tables must live on the HIP device"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))


# ---------------------------------------------------------------- C ABI
def test_struct_layout_agrees_with_header():
    from pykg2vec_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    body = re.search(r"typedef struct kge_acre_desc \{(.*?)\} kge_acre_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", x).strip(" *\n") for x in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    D = _lib.AcreDesc
    assert names == [f[0] for f in D._fields_]
    assert names[18:37] == list(_lib.ACRE_TABLES_PARALLEL) and names[18] == "bias"      # state-dict order: the bare parameter first
    assert _lib.ACRE_TABLES_PARALLEL[:17] == _lib.ACRE_TABLES_SERIAL and _lib.ACRE_TABLES_PARALLEL[17:] == ("gate_w", "gate_b")
    assert _lib.ACRE_BUFFERS == ("bn0_mean", "bn0_var", "bn1_mean", "bn1_var", "bn2_mean", "bn2_var")
    # 2 x int64, 7 x int32, 3 x float, 2 x int32, 2 x uint64, 6 x float, 19 + 6 + 19 pointers: no padding
    assert ctypes.sizeof(D) == 16 + 28 + 12 + 8 + 16 + 24 + 44 * 8 == 456
    assert D.hidden_size.offset == 16 and D.way.offset == 24 and D.third_atrous.offset == 36 and D.acre_bias.offset == 40
    assert D.input_dropout.offset == 44 and D.train.offset == 56 and D.seed.offset == 64 and D.eps.offset == 80 and D.momentum.offset == 92
    assert D.bias.offset == 104 and D.gate_b.offset == 248 and D.bn0_mean.offset == 256 and D.g_bias.offset == 304 and D.g_gate_b.offset == 448
    for off in re.findall(r"(\d+) (\w+)", re.search(r"layout \(no padding\): (.*?) the 19 tables", body_with_comments(header), re.S).group(1)):
        if hasattr(D, off[1]):
            assert getattr(D, off[1]).offset == int(off[0]), off
    assert re.search(r"#define KGE_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3      # untouched
    assert re.search(r"#define KGE_ACRE_MAX_CHANNELS %d\b" % _lib.ACRE_MAX_CHANNELS, header) and _lib.ACRE_MAX_CHANNELS >= 32
    assert re.search(r"#define KGE_ACRE_MAX_ATROUS %d\b" % _lib.ACRE_MAX_ATROUS, header) and _lib.ACRE_MAX_ATROUS >= 4


def body_with_comments(header):
    return re.search(r"typedef struct kge_acre_desc \{(.*?)\} kge_acre_desc;", header, re.S).group(1)


SYMBOLS = ["kge_acre_saved_floats", "kge_acre_body_forward", "kge_acre_body_backward", "kge_acre_train_bce", "kge_acre_eval_ranks"] + \
          ["kge_acre_%s_workspace_bytes" % s for s in ("body_forward", "body_backward", "train_bce", "eval_ranks")]


def test_symbols_are_exported():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


def _desc(C=3, bias=True):
    from pykg2vec_amd import _lib
    d = _lib.AcreDesc()
    d.tot_entity, d.tot_relation, d.hidden_size, d.in_channels, d.way, d.train = 10, 3, 200, C, 0, 1
    d.first_atrous, d.second_atrous, d.third_atrous, d.acre_bias = 1, 2, 3, int(bias)
    for i in range(3):
        d.eps[i], d.momentum[i] = 1e-5, 0.1
    names = [n for n in _lib.ACRE_TABLES_SERIAL if bias or not n.endswith("_b") or not n.startswith("conv")]
    for f in tuple(names) + _lib.ACRE_BUFFERS + tuple("g_" + n for n in names):
        setattr(d, f, 0x1000)    # never dereferenced: every call below is refused before a launch
    return d


def _set(d, field, value):
    if isinstance(field, tuple):
        getattr(d, field[0])[field[1]] = value
    else:
        setattr(d, field, value)


@pytest.mark.parametrize("field,value,msg", [
    ("ent", None, "null tables"), ("bias", None, "null tables"), ("conv2_w", None, "null tables"), ("bn2_var", None, "null tables"),
    ("tot_entity", 0, "must be positive"), ("tot_relation", 0, "must be positive"), ("in_channels", 0, "must be positive"),
    ("hidden_size", -1, "must be positive"), ("hidden_size", 100, "hidden_size = 100 must be 200"),
    ("way", 2, "way = 2 must be 0 (serial) or 1 (parallel)"), ("way", -1, "way = -1 must be 0"),
    ("first_atrous", 0, "dilation 1 = 0 must be in [1, 4]"), ("third_atrous", 5, "dilation 3 = 5 must be in [1, 4]"),
    ("in_channels", 33, "in_channels = 33 exceeds 32"),
    ("conv2_b", None, "convolution bias pointers must all be set with acre_bias = 1"),
    ("acre_bias", 0, "all be NULL with acre_bias = 0"),
    ("gate_w", 0x1000, "gate pointers must both be set in the parallel way and both be NULL in the serial way"),
    ("way", 1, "gate pointers must both be set in the parallel way"),
    (("momentum", 1), 0.0, "momentum 1 must be in (0, 1]"), (("momentum", 2), 1.5, "momentum 2 must be in (0, 1]"),
    (("eps", 0), -1.0, "eps 0 must not be negative"),
    ("feature_map_dropout", 1.0, "dropout rate 1"), ("input_dropout", -0.1, "dropout rate 0"), ("offset", 1 << 62, "offset"),
    ("g_conv1_w", None, "null gradient buffers"), ("g_conv3_b", None, "null gradient buffers")])
def test_entry_points_refuse_bad_descriptors(field, value, msg):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    _set(d, field, value)
    p = ctypes.c_void_p(0x1000)
    rc = lib.kge_acre_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, 1 << 40, p, None)
    assert rc != 0 and msg in lib.kge_last_error().decode() and "kge_acre_train_bce" in lib.kge_last_error().decode()
    assert lib.kge_acre_train_bce_workspace_bytes(ctypes.byref(d), 4, 1, 1) == 0 or str(field).startswith("g_")
    if not str(field).startswith("g_"):
        assert lib.kge_acre_body_forward_workspace_bytes(ctypes.byref(d), 4) == 0
        assert "kge_acre_body_forward_workspace_bytes" in lib.kge_last_error().decode()
        assert lib.kge_acre_body_backward_workspace_bytes(ctypes.byref(d), 4) == 0
        assert lib.kge_acre_eval_ranks_workspace_bytes(ctypes.byref(d), 4) == 0
        assert lib.kge_acre_saved_floats(ctypes.byref(d), 4) == 0
        assert lib.kge_acre_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, 1 << 40, p, None, None) != 0
        assert "kge_acre_eval_ranks" in lib.kge_last_error().decode() and msg in lib.kge_last_error().decode()
        assert lib.kge_acre_body_forward(ctypes.byref(d), p, p, 4, 0, p, p, p, 1 << 40, None) != 0
        assert "kge_acre_body_forward" in lib.kge_last_error().decode()
    assert lib.kge_acre_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, p, 1 << 40, None) != 0
    assert "kge_acre_body_backward" in lib.kge_last_error().decode() and msg in lib.kge_last_error().decode()


def test_smallest_and_largest_sizes_are_accepted():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    for C in (1, 3, _lib.ACRE_MAX_CHANNELS):
        for bias in (True, False):
            d = _desc(C, bias)
            for a in (1, _lib.ACRE_MAX_ATROUS):
                d.first_atrous = d.second_atrous = d.third_atrous = a
                # saved: c, z1, z2 [n, 400 C] | u [n, 200] | the feature-map factors [n, C] | the statistics 2 + 2 C + 400
                assert lib.kge_acre_saved_floats(ctypes.byref(d), 4) == 4 * (3 * 400 * C + 200 + C) + 2 + 2 * C + 400
                assert lib.kge_acre_body_forward_workspace_bytes(ctypes.byref(d), 4) > 0
                assert lib.kge_acre_body_backward_workspace_bytes(ctypes.byref(d), 4) > 0
                assert lib.kge_acre_eval_ranks_workspace_bytes(ctypes.byref(d), 4) > 0
    # the five presets: serial, C = 32, dilations 1 / 2 / 2, batch 128 or 256
    d = _desc(32, True)
    d.tot_entity, d.tot_relation, d.first_atrous, d.second_atrous, d.third_atrous = 14951, 1345, 1, 2, 2
    for B in (128, 256):
        assert lib.kge_acre_saved_floats(ctypes.byref(d), B) == B * (3 * 12800 + 200 + 32) + 2 + 64 + 400
        assert lib.kge_acre_train_bce_workspace_bytes(ctypes.byref(d), B, 1000, 1000) > 0


def test_entry_points_refuse_one_training_row_small_workspaces_and_eval_backward():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    p = ctypes.c_void_p(0x1000)
    big = 1 << 40
    assert lib.kge_acre_body_forward(ctypes.byref(d), p, p, 1, 0, p, p, p, big, None) != 0
    assert "kge_acre_body_forward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_acre_body_backward(ctypes.byref(d), p, p, 1, 0, p, p, p, big, None) != 0
    assert "kge_acre_body_backward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_acre_train_bce(ctypes.byref(d), p, p, p, 1, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "kge_acre_train_bce" in lib.kge_last_error().decode() and "needs more than one row" in lib.kge_last_error().decode()
    need = lib.kge_acre_body_forward_workspace_bytes(ctypes.byref(d), 4)
    assert need > 0
    assert lib.kge_acre_body_forward(ctypes.byref(d), p, p, 4, 0, p, p, p, need - 1, None) != 0
    assert "kge_acre_body_forward: workspace too small" in lib.kge_last_error().decode()
    assert lib.kge_acre_body_forward(ctypes.byref(d), p, p, 4, -1, p, p, p, need, None) != 0 and "row0 + n below 2^32" in lib.kge_last_error().decode()
    assert lib.kge_acre_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, None, 0, None) != 0
    assert "kge_acre_body_backward: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_acre_train_bce_workspace_bytes(ctypes.byref(d), 4, 1, 1)
    assert lib.kge_acre_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, need - 1, p, None) != 0
    assert "kge_acre_train_bce: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_acre_eval_ranks_workspace_bytes(ctypes.byref(d), 4)
    assert lib.kge_acre_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, need - 1, p, None, None) != 0
    assert "kge_acre_eval_ranks: workspace too small" in lib.kge_last_error().decode()
    d.train = 0
    assert lib.kge_acre_body_forward_workspace_bytes(ctypes.byref(d), 1) > 0      # one row is fine in the eval form
    assert lib.kge_acre_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, p, big, None) != 0
    assert "kge_acre_body_backward: the eval form (train = 0) has no backward" in lib.kge_last_error().decode()
    assert lib.kge_acre_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "kge_acre_train_bce: the step is the training form" in lib.kge_last_error().decode()


def test_python_level_refusals_need_no_device():
    from pykg2vec_amd import _lib as L, kernels as K
    m = build()
    m.bn1.momentum = None
    with pytest.raises(L.KgeHipError, match="cumulative moving average"):
        m.make_desc()
    m.bn1.momentum = 0.1
    with pytest.raises(L.KgeHipError, match="acre: 17 tensors and 6 running buffers expected"):
        K.acre_desc(m.trainable_tensors()[:-1], m.running_buffers(), tot_entity=70, tot_relation=5, in_channels=3)
    with pytest.raises(L.KgeHipError, match="acre: way must be 'serial' or 'parallel'"):
        K.acre_desc(m.trainable_tensors(), m.running_buffers(), tot_entity=70, tot_relation=5, in_channels=3, way="both")
    with pytest.raises(L.KgeHipError, match=r"acre: bn1_w must be \(4,\)"):
        K.acre_desc(m.trainable_tensors(), m.running_buffers(), tot_entity=70, tot_relation=5, in_channels=4)
    with pytest.raises(L.KgeHipError, match=r"acre: rel_embeddings must be \[>= 12, 200\]"):
        K.acre_desc(m.trainable_tensors(), m.running_buffers(), tot_entity=70, tot_relation=6, in_channels=3)
    names, shapes, bufs = K.acre_shapes(70, 5, 3, 0, True)
    assert tuple(names) == L.ACRE_TABLES_SERIAL and shapes[9] == (200, 1200) and shapes[13] == (3, 3, 3, 3) and bufs[0] == (1,)
    assert tuple(K.acre_shapes(70, 5, 3, 1, True)[0]) == L.ACRE_TABLES_PARALLEL and K.acre_shapes(70, 5, 3, 1, True)[1][13] == (3, 1, 3, 3)
