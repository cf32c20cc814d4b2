"""InteractE without a GPU: the float64 restatement (tools/interacte_reference.py) reproduces the live reference's float64 outputs frozen
in tests/golden/ref_interacte{,_ls,_masked}.npz (1e-10, ranks exact), the recorded Philox masks and the recorded chequer permutation;
the drop-in class keeps the reference's construction contract, state dict and np.random draw; every refusal that needs no device raises
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
from tools import interacte_reference as ir  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["interacte", "interacte_ls", "interacte_masked"]
TENSORS, BUFFERS, COUNTERS = ir.TENSORS, ir.BUFFERS, ir.COUNTERS
PARAMS = dict(tot_entity=70, tot_relation=5, hidden_size=6, input_dropout=0.2, hidden_dropout=0.3, feature_map_dropout=0.2,
              feature_permutation=2, num_filters=3, kernel_size=3, reshape_height=3, reshape_width=2)
# the reference's state dict, in its order: the bare parameters bias and conv_filt first, then the modules in registration order
SHAPES = [("bias", (70,)), ("conv_filt", (3, 1, 3, 3)), ("ent_embeddings.weight", (70, 6)), ("rel_embeddings.weight", (5, 6)),
          ("bn0.weight", (2,)), ("bn0.bias", (2,)), ("bn0.running_mean", (2,)), ("bn0.running_var", (2,)), ("bn0.num_batches_tracked", ()),
          ("bn1.weight", (6,)), ("bn1.bias", (6,)), ("bn1.running_mean", (6,)), ("bn1.running_var", (6,)), ("bn1.num_batches_tracked", ()),
          ("bn2.weight", (6,)), ("bn2.bias", (6,)), ("bn2.running_mean", (6,)), ("bn2.running_var", (6,)), ("bn2.num_batches_tracked", ()),
          ("fc.weight", (6, 72)), ("fc.bias", (6,))]
RTOL = 1e-10


def fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)))
    z["ls"] = None if z["label_smoothing"] < 0 else float(z["label_smoothing"])
    z["rates"] = tuple(float(p) for p in z["dropouts"])
    z["masked"] = "mask_seed" in z
    z["G"] = {k: z[k] for k in ("reshape_height", "reshape_width", "feature_permutation", "num_filters", "kernel_size", "chequer_perm")}
    return z


def tables(z):
    """The restatement's view of a fixture's state before the step."""
    return {k: z[k].astype(np.float64) for k in TENSORS + BUFFERS}


def recorded_masks(z):
    return [tuple(z["mask.%s.%d" % (d, s)] for s in range(3)) for d in ("tail", "head")] if z["masked"] else None


def state_dict_of(z):
    return {k: torch.from_numpy(np.asarray(z[k])) for k, _ in SHAPES}


def build(**over):
    from pykg2vec_amd.projection import InteractE
    kw = dict(PARAMS)
    kw.update(over)
    return InteractE(**kw)


def close(got, want, scale=None):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want).max() <= RTOL * max(np.abs(want).max(), scale or 0.0)


# ---------------------------------------------------------------- the restatement against the live reference
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_float64(name):
    z = fixture(name)
    P, G = tables(z), z["G"]
    out = ir.step(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"], mask_list=recorded_masks(z))
    assert abs(out["loss"] - z["loss"]) <= RTOL * abs(z["loss"])
    assert close(out["pred_tails"], z["pred_tails"]) and close(out["pred_heads"], z["pred_heads"])
    vanishing = ir.VANISHING(z["rates"], P["bn0.bias"])
    for k in TENSORS:
        # a gradient that vanishes analytically is rounding noise on both sides: compared on its cancellation scale
        assert close(out["grads"][k], z["grad." + k], out["scale"][k] if k in vanishing else None), k
    for k in BUFFERS:
        assert close(out["buffers"][k], z["after." + k]), k
        assert not np.array_equal(z["after." + k], z[k]), k     # the step moved every running buffer
    for k in COUNTERS:
        assert int(z["after." + k]) == int(z[k]) + 2 and int(z[k]) == 2
    assert out["margin"] > 1e-5 and ir.eval_margin(P, G, z["test"]) > 1e-5     # bn1 and bn2 both feed a relu
    assert close(ir.forward(P, G, z["h"], z["r"], "tail"), z["eval_pred_tails"])
    assert close(ir.forward(P, G, z["t"], z["r"], "head"), z["eval_pred_heads"])
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    ranks, gap = ir.ranks(P, G, z["test"], known)
    assert np.array_equal(ranks, z["ranks"]) and gap > 1e-6
    # no padding_idx: id 0 of both tables is in the batch and its lookup gradient is an ordinary row
    assert (z["h"] == 0).sum() == 1 and (z["t"] == 0).sum() == 1 and (z["r"] == 0).any() and (z["test"] == 0).any()
    assert np.abs(z["grad.rel_embeddings.weight"][0]).max() > 0


def test_vanishing_rule_follows_the_rates():
    assert ir.VANISHING((0.0, 0.0, 0.0)) == ("fc.bias", "bn0.bias", "bn0.weight")
    assert ir.VANISHING((0.0, 0.2, 0.0)) == ("fc.bias", "bn0.bias", "bn0.weight")
    assert ir.VANISHING((0.2, 0.2, 0.0)) == ("fc.bias",)
    assert ir.VANISHING((0.2, 0.2, 0.3), np.array([0.25, 0.0])) == ()
    assert ir.VANISHING((0.2, 0.2, 0.3), np.zeros(2)) == ("bn0.weight",)
    z = fixture("interacte")
    big = np.abs(z["grad.bn1.weight"]).max()
    for k in ("fc.bias", "bn0.bias"):     # zero analytically: the circular padding makes bn0.bias a constant per conv channel
        assert np.abs(z["grad." + k]).max() < 1e-9 * big, k
    assert np.abs(z["grad.bn0.weight"]).max() < 1e-4 * big     # survives through bn1's eps alone
    assert np.abs(z["grad.bn1.bias"]).max() > 1e-4 * big       # the relu after bn1 keeps it alive, unlike HypER's
    z = fixture("interacte_masked")
    for k in ("fc.bias", "bn0.bias", "bn0.weight"):
        assert np.abs(z["grad." + k]).max() > 1e-4 * big, k


def test_restatement_masks_are_the_recorded_masks():
    z = fixture("interacte_masked")
    B = len(z["h"])
    for side, want in enumerate(recorded_masks(z)):
        got = ir.masks(B, z["G"], z["rates"], int(z["mask_seed"]), int(z["mask_offset"]), row0=side * B)
        for site in range(3):
            assert np.array_equal(got[site], want[site]), (side, site)
            p = np.float32(z["rates"][site])
            assert set(np.unique(want[site])) == {0.0, float(np.float32(1) / (np.float32(1) - p))}
    assert [m.shape for m in recorded_masks(z)[0]] == [(B, 2, 4, 3), (B, 6), (B, 6)]      # H = 2 reshape_width = 4, W = reshape_height = 3
    assert not np.array_equal(z["mask.tail.0"], z["mask.head.0"])
    assert np.array_equal(ir.masks(2 * B, z["G"], z["rates"], int(z["mask_seed"]), int(z["mask_offset"]))[1][B:], z["mask.head.1"])


def test_circular_convolution_and_shared_filter():
    """The restated convolution against a direct loop with explicit modular indices, and the eval form's bn2."""
    z = fixture("interacte")
    P, G = tables(z), z["G"]
    k, H, W, NP, NF, ks, pad, C, F, perm = ir.geometry(G)
    assert (H, W) == (4, 3) and F == 72
    x, s, stats = ir.body(P, G, z["h"], z["r"], train=False)
    comb = np.concatenate([P["ent_embeddings.weight"][z["h"]], P["rel_embeddings.weight"][z["r"]]], 1)
    img = comb[:, perm].reshape(-1, NP, H, W)
    y0 = (img - P["bn0.running_mean"][None, :, None, None]) / np.sqrt(P["bn0.running_var"][None, :, None, None] + 1e-5) \
        * P["bn0.weight"][None, :, None, None] + P["bn0.bias"][None, :, None, None]
    c = np.zeros((len(z["h"]), C, H, W))
    for p in range(NP):
        for f in range(NF):
            for y in range(H):
                for xx in range(W):
                    for i in range(ks):
                        for j in range(ks):
                            c[:, p * NF + f, y, xx] += P["conv_filt"][f, 0, i, j] * y0[:, p, (y + i - pad) % H, (xx + j - pad) % W]
    y1 = (c - P["bn1.running_mean"][None, :, None, None]) / np.sqrt(P["bn1.running_var"][None, :, None, None] + 1e-5) \
        * P["bn1.weight"][None, :, None, None] + P["bn1.bias"][None, :, None, None]
    assert np.abs(y1 - s["y1"]).max() < 1e-12
    want = (s["u"] - P["bn2.running_mean"]) / np.sqrt(P["bn2.running_var"] + 1e-5) * P["bn2.weight"] + P["bn2.bias"]
    assert np.array_equal(x, np.maximum(want, 0)) and stats == {}
    with pytest.raises(ValueError, match="more than 1 value"):
        ir.body(P, G, z["h"][:1], z["r"][:1], train=True)
    assert np.array_equal(ir.forward(P, G, z["h"], z["r"], "tail"), ir.forward(P, G, z["h"], z["r"], "head"))


# ---------------------------------------------------------------- the drop-in class
@pytest.mark.parametrize("missing", sorted(PARAMS))
def test_constructor_names_the_missing_parameter(missing):
    from pykg2vec_amd.projection import InteractE
    kw = {k: v for k, v in PARAMS.items() if k != missing}
    with pytest.raises(Exception, match="hyperparameter %s not found" % missing):
        InteractE(**kw)


def test_class_contract_and_state_dict():
    import pykg2vec_amd as pa
    from pykg2vec_amd import TrainingStrategy, import_model
    from pykg2vec_amd.criterion import Criterion
    from pykg2vec_amd.kgmeta import ProjectionModel
    m = build(device="cpu")
    assert pa.MODEL_MAP["interacte"] == "projection.InteractE"
    assert import_model("interacte") is type(m) and isinstance(m, ProjectionModel) and m.kernel_name == "interacte" and m.device == "cpu"
    assert build().device == torch.device("cpu")
    assert m.model_name == "interacte" and m.training_strategy == TrainingStrategy.PROJECTION_BASED
    assert m.loss is Criterion.multi_class_bce and m.get_reg(None, None, None) == 0
    assert m.parameter_list == [m.ent_embeddings, m.rel_embeddings]
    assert m.ent_embeddings.padding_idx is None and m.rel_embeddings.padding_idx is None
    assert m.hidden_size == 6 and build(hidden_size=999).hidden_size == 6      # reshape_width * reshape_height, whatever was passed
    assert m.flat_sz == 72
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == SHAPES          # keys, ORDER and shapes
    assert "chequer_perm" not in sd and len(list(m.parameters())) == 12
    z = fixture("interacte")
    assert [str(k) for k in z["state_keys"]] == [k for k, _ in SHAPES]      # the live reference's state dict: the same keys in the same order
    assert [np.asarray(z[k]).shape for k, _ in SHAPES] == [s for _, s in SHAPES]
    m.load_state_dict(state_dict_of(z), strict=True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), z[k]), k
    assert int(m.bn1.num_batches_tracked) == 2
    tt = m.trainable_tensors()
    named = dict(m.named_parameters())
    assert list(named) == list(TENSORS)
    assert len(tt) == 12 and all(t is named[k] for t, k in zip(tt, TENSORS)) and tt[0] is m.bias and tt[1] is m.conv_filt
    assert [tuple(b.shape) for b in m.running_buffers()] == [dict(SHAPES)[k] for k in BUFFERS]
    with pytest.raises(AssertionError, match="Unknown forward direction"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), direction="sideways")
    e1, r1, e2 = m.embed(torch.tensor([1]), torch.tensor([4]), torch.tensor([2]))
    assert e1.shape == e2.shape == r1.shape == (1, 6) and torch.equal(m.embed2(torch.tensor([1]), torch.tensor([4]))[1], r1)


@pytest.mark.parametrize("name", NAMES)
def test_chequer_perm_is_the_reference_s_draw(name):
    z = fixture(name)
    np.random.seed(int(z["np_seed"]))
    m = build()
    assert m.chequer_perm.dtype == torch.int64 and tuple(m.chequer_perm.shape) == (2, 12)
    assert np.array_equal(m.chequer_perm.numpy(), z["chequer_perm"])
    assert np.array_equal(ir.chequer_perm(z["G"], int(z["np_seed"])), z["chequer_perm"])
    # both parities of the chequer pattern: permutation 0 starts with an entity value, permutation 1 with a relation value
    assert z["chequer_perm"][0, 0] < 6 <= z["chequer_perm"][0, 1] and z["chequer_perm"][1, 0] >= 6 > z["chequer_perm"][1, 1]
    for p in range(2):
        assert sorted(z["chequer_perm"][p].tolist()) == list(range(12))


def test_perm_is_checked_inverted_and_cached():
    from pykg2vec_amd import _lib
    from pykg2vec_amd import kernels as K
    z = fixture("interacte")
    m = build()
    m.chequer_perm = torch.from_numpy(z["chequer_perm"])      # loading a reference model's permutation
    perm, inv = m._perms()
    assert perm.dtype == inv.dtype == torch.int32 and np.array_equal(perm.numpy(), z["chequer_perm"])
    for p in range(2):
        assert np.array_equal(inv[p].numpy()[z["chequer_perm"][p]], np.arange(12))
    assert m._perms()[0] is perm                                # cached
    m.chequer_perm = m.chequer_perm.flip(1)
    assert m._perms()[0] is not perm and np.array_equal(m._perms()[0].numpy(), z["chequer_perm"][:, ::-1])      # rebuilt on reassignment
    first = m._perms()[0]
    m.chequer_perm[0, :2] = m.chequer_perm[0, :2].flip(0)       # ... and on a change in place
    assert m._perms()[0] is not first
    bad = torch.from_numpy(z["chequer_perm"]).clone()
    bad[1, 3] = bad[1, 4]                                       # a repeated index
    m.chequer_perm = bad
    with pytest.raises(_lib.KgeHipError, match=r"row 1 of chequer_perm is not a permutation of \[0, 12\)"):
        m.make_desc()
    bad = torch.from_numpy(z["chequer_perm"]).clone()
    bad[0, 0] = 12                                              # out of range: would be an out-of-bounds read on the device
    m.chequer_perm = bad
    with pytest.raises(_lib.KgeHipError, match="row 0 of chequer_perm is not a permutation"):
        m.make_desc()
    with pytest.raises(_lib.KgeHipError, match="chequer_perm must be an integer tensor of shape"):
        K.interacte_perm(torch.zeros(2, 11, dtype=torch.long), 2, 6, "cpu")


def test_default_init_is_the_reference_s():
    """xavier_uniform_ on both tables and conv_filt, bias zero, torch's defaults elsewhere."""
    torch.manual_seed(0)
    m = build(tot_entity=4000, num_filters=64, kernel_size=9)
    for w in (m.ent_embeddings.weight.detach(), m.rel_embeddings.weight.detach()):
        bound = (6.0 / (w.shape[0] + w.shape[1])) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
        assert float(w[0].abs().min()) > 0
    w = m.conv_filt.detach()
    bound = (6.0 / (81 * (1 + 64))) ** 0.5      # fan_in = 1 * 81, fan_out = 64 * 81
    assert w.shape == (64, 1, 9, 9) and float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    assert m.bias.shape == (4000,) and float(m.bias.detach().abs().max()) == 0.0 and isinstance(m.bias, torch.nn.Parameter)
    assert float(m.bn1.weight.min()) == 1.0 and float(m.bn1.running_var.min()) == 1.0 and m.bn0.momentum == 0.1 and m.bn2.eps == 1e-5
    assert m.bn0.num_features == 2 and m.bn1.num_features == 128 and m.fc.in_features == 128 * 12


def test_cpu_tensors_are_refused():
    m = build()
    with pytest.raises(Exception, match="kge::interacte_body: ids and tables must live on the HIP device"):
        m.forward(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))


# ---------------------------------------------------------------- C ABI
def test_struct_layout_agrees_with_header():
    from pykg2vec_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    body = re.search(r"typedef struct kge_interacte_desc \{(.*?)\} kge_interacte_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", x).strip(" *") for x in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    D = _lib.InteracteDesc
    assert names == [f[0] for f in D._fields_]
    assert names[18:30] == list(_lib.INTERACTE_TABLES) and names[18:20] == ["bias", "conv_filt"]      # state-dict order: the bare parameters first
    # 2 x int64, 5 x int32, 3 x float, 2 x int32, 2 x uint64, 6 x float, 2 + 30 pointers: no padding
    assert ctypes.sizeof(D) == 16 + 20 + 12 + 8 + 16 + 24 + 32 * 8 == 352
    assert D.kernel_size.offset == 32 and D.train.offset == 48 and D.seed.offset == 56 and D.eps.offset == 72 and D.perm.offset == 96
    assert D.bias.offset == 112 and D.bn0_mean.offset == 112 + 12 * 8 and D.g_bias.offset == 112 + 18 * 8
    assert re.search(r"#define KGE_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3      # untouched
    assert re.search(r"#define KGE_INTERACTE_MAX_HIDDEN %d\b" % _lib.INTERACTE_MAX_HIDDEN, header) and _lib.INTERACTE_MAX_HIDDEN >= 200
    assert re.search(r"#define KGE_INTERACTE_MAX_KERNEL %d\b" % _lib.INTERACTE_MAX_KERNEL, header) and _lib.INTERACTE_MAX_KERNEL >= 11
    assert re.search(r"#define KGE_INTERACTE_MAX_FLAT \(1 << 22\)", header) and _lib.INTERACTE_MAX_FLAT == 1 << 22


SYMBOLS = ["kge_interacte_saved_floats", "kge_interacte_body_forward", "kge_interacte_body_backward", "kge_interacte_train_bce",
           "kge_interacte_eval_ranks"] + \
          ["kge_interacte_%s_workspace_bytes" % s for s in ("body_forward", "body_backward", "train_bce", "eval_ranks")]


def test_symbols_are_exported():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


def _desc():
    from pykg2vec_amd import _lib
    d = _lib.InteracteDesc()
    d.tot_entity, d.tot_relation, d.reshape_height, d.reshape_width, d.train = 10, 3, 3, 2, 1
    d.feature_permutation, d.num_filters, d.kernel_size = 2, 3, 3
    for i in range(3):
        d.eps[i], d.momentum[i] = 1e-5, 0.1
    for f in ("perm", "inv_perm") + _lib.INTERACTE_TABLES + _lib.INTERACTE_BUFFERS + tuple("g_" + n for n in _lib.INTERACTE_TABLES):
        setattr(d, f, 0x1000)    # never dereferenced: every call below is refused before a launch
    return d


def _set(d, field, value):
    if isinstance(field, tuple):
        getattr(d, field[0])[field[1]] = value
    else:
        setattr(d, field, value)


@pytest.mark.parametrize("field,value,msg", [
    ("ent", None, "null tables"), ("bias", None, "null tables"), ("conv_filt", None, "null tables"), ("bn2_var", None, "null tables"),
    ("perm", None, "null perm / inv_perm"), ("inv_perm", None, "null perm / inv_perm"),
    ("reshape_height", 0, "must be positive"), ("reshape_width", -1, "must be positive"), ("feature_permutation", 0, "must be positive"),
    ("num_filters", 0, "must be positive"), ("kernel_size", 0, "must be positive"), ("tot_relation", 0, "must be positive"),
    ("kernel_size", 4, "kernel_size = 4 must be odd and at least 3"), ("kernel_size", 1, "kernel_size = 1 must be odd and at least 3"),
    ("kernel_size", 13, "kernel_size = 13 exceeds 11"),
    ("kernel_size", 9, "kernel_size / 2 = 4 exceeds min(H, W) = 3 of the 4 x 3 image"),
    ("reshape_height", 257, "reshape_height * reshape_width = 514 exceeds 512"),
    ("num_filters", 1 << 20, "exceeds 4194304"),
    (("momentum", 1), 0.0, "momentum 1 must be in (0, 1]"), (("momentum", 2), 1.5, "momentum 2 must be in (0, 1]"),
    (("eps", 0), -1.0, "eps 0 must not be negative"),
    ("feature_map_dropout", 1.0, "dropout rate 1"), ("input_dropout", -0.1, "dropout rate 0"), ("offset", 1 << 62, "offset"),
    ("g_conv_filt", None, "null gradient buffers")])
def test_entry_points_refuse_bad_descriptors(field, value, msg):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    _set(d, field, value)
    p = ctypes.c_void_p(0x1000)
    rc = lib.kge_interacte_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, 1 << 40, p, None)
    assert rc != 0 and msg in lib.kge_last_error().decode() and "kge_interacte_train_bce" in lib.kge_last_error().decode()
    if field != "g_conv_filt":
        assert lib.kge_interacte_body_forward_workspace_bytes(ctypes.byref(d), 4) == 0
        assert "kge_interacte_body_forward_workspace_bytes" in lib.kge_last_error().decode()
        assert lib.kge_interacte_saved_floats(ctypes.byref(d), 4) == 0
        assert lib.kge_interacte_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, 1 << 40, p, None, None) != 0
        assert "kge_interacte_eval_ranks" in lib.kge_last_error().decode() and msg in lib.kge_last_error().decode()
        assert lib.kge_interacte_body_forward(ctypes.byref(d), p, p, 4, 0, p, p, p, 1 << 40, None) != 0
        assert "kge_interacte_body_forward" in lib.kge_last_error().decode()
    assert lib.kge_interacte_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, p, 1 << 40, None) != 0
    assert "kge_interacte_body_backward" in lib.kge_last_error().decode() and msg in lib.kge_last_error().decode()


def test_smallest_and_largest_sizes_are_accepted():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    d.reshape_height, d.reshape_width, d.feature_permutation, d.num_filters, d.kernel_size = 1, 1, 1, 1, 3      # a 2 x 1 image, pad 1 = min(H, W)
    assert lib.kge_interacte_saved_floats(ctypes.byref(d), 4) == 4 * (2 + 1 + 1) + 2 + 2 + 2
    d.reshape_height, d.reshape_width, d.kernel_size = 3, 2, 7      # pad = 3 = min(H, W): the largest wrap
    assert lib.kge_interacte_body_forward_workspace_bytes(ctypes.byref(d), 4) > 0
    for rh, rw in ((256, 2), (2, 256), (512, 1), (1, 512), (16, 32)):      # K = 512 in every aspect the padded LDS image must hold
        d.reshape_height, d.reshape_width = rh, rw
        for ks in (3, 11):
            d.kernel_size = ks
            ok = ks // 2 <= min(2 * rw, rh)
            assert (lib.kge_interacte_body_backward_workspace_bytes(ctypes.byref(d), 4) > 0) == ok, (rh, rw, ks)
    # the four presets: (P, NF, ks) at reshape 20 x 10
    d.reshape_height, d.reshape_width = 20, 10
    for P, NF, ks in ((1, 96, 9), (2, 96, 11), (4, 64, 7)):
        d.feature_permutation, d.num_filters, d.kernel_size = P, NF, ks
        assert lib.kge_interacte_saved_floats(ctypes.byref(d), 128) == 128 * (P * NF * 400 + 200 + P * NF) + 2 * P + 2 * P * NF + 400
        assert lib.kge_interacte_train_bce_workspace_bytes(ctypes.byref(d), 128, 1000, 1000) > 0


def test_entry_points_refuse_one_training_row_small_workspaces_and_eval_backward():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    p = ctypes.c_void_p(0x1000)
    big = 1 << 40
    assert lib.kge_interacte_body_forward(ctypes.byref(d), p, p, 1, 0, p, p, p, big, None) != 0
    assert "kge_interacte_body_forward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_interacte_body_backward(ctypes.byref(d), p, p, 1, 0, p, p, p, big, None) != 0
    assert "kge_interacte_body_backward: batch norm in training form needs more than one row" in lib.kge_last_error().decode()
    assert lib.kge_interacte_train_bce(ctypes.byref(d), p, p, p, 1, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "kge_interacte_train_bce" in lib.kge_last_error().decode() and "needs more than one row" in lib.kge_last_error().decode()
    need = lib.kge_interacte_body_forward_workspace_bytes(ctypes.byref(d), 4)
    assert need > 0
    assert lib.kge_interacte_body_forward(ctypes.byref(d), p, p, 4, 0, p, p, p, need - 1, None) != 0
    assert "kge_interacte_body_forward: workspace too small" in lib.kge_last_error().decode()
    assert lib.kge_interacte_body_forward(ctypes.byref(d), p, p, 4, -1, p, p, p, need, None) != 0 and "row0 + n below 2^32" in lib.kge_last_error().decode()
    assert lib.kge_interacte_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, None, 0, None) != 0
    assert "kge_interacte_body_backward: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_interacte_train_bce_workspace_bytes(ctypes.byref(d), 4, 1, 1)
    assert lib.kge_interacte_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, need - 1, p, None) != 0
    assert "kge_interacte_train_bce: workspace too small" in lib.kge_last_error().decode()
    need = lib.kge_interacte_eval_ranks_workspace_bytes(ctypes.byref(d), 4)
    assert lib.kge_interacte_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, need - 1, p, None, None) != 0
    assert "kge_interacte_eval_ranks: workspace too small" in lib.kge_last_error().decode()
    d.train = 0
    assert lib.kge_interacte_body_forward_workspace_bytes(ctypes.byref(d), 1) > 0      # one row is fine in the eval form
    assert lib.kge_interacte_body_backward(ctypes.byref(d), p, p, 4, 0, p, p, p, big, None) != 0
    assert "kge_interacte_body_backward: the eval form (train = 0) has no backward" in lib.kge_last_error().decode()
    assert lib.kge_interacte_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, big, p, None) != 0
    assert "kge_interacte_train_bce: the step is the training form" in lib.kge_last_error().decode()
