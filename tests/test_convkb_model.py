"""ConvKB without a GPU: the drop-in class keeps the reference's construction contract (pinned by the key names inside
tests/golden/ref_convkb*.npz, which come from the live reference), the float64 restatement of the collapsed affine form and its
gradient formulas (tools/convkb_reference.py) reproduces the frozen reference outputs -- which validates the fixture and the math
the kernels implement --, every kge_convkb_* entry point refuses bad descriptors before any launch, and the ctypes struct agrees
with the header."""
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
from tools import convkb_reference as cr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["convkb", "convkb_neg3"]
TRAINED = ("ent_embeddings.weight", "rel_embeddings.weight", "fc1.weight", "fc1.bias")
GRAD_TOL = dict(atol=2e-5, rtol=1e-4)      # the project's fixture tolerances (tests/test_hip_octonione.py)
SCORE_TOL = dict(atol=2e-5, rtol=2e-5)


class ConvCase:
    """golden_util.Case for the ConvKB fixtures (its hyper-parameters include a list, filter_sizes)."""

    def __init__(self, name):
        self.name, self.model, self.pointwise = name, "convkb", True
        self.z = z = dict(np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)))
        self.E, self.R, self.B = int(z["E"]), int(z["R"]), int(z["B"])
        self.hp = {k[3:]: (z[k].tolist() if z[k].ndim else z[k].item()) for k in z if k.startswith("hp_")}
        self.train, self.valid, self.test = z["train"], z["valid"], z["test"]
        self.n_filters = len(self.hp["filter_sizes"])

    def batch(self, s):
        return tuple(self.z["batch%d.%d" % (s, i)] for i in range(4))

    def filters(self):
        allt = np.concatenate([self.train, self.valid, self.test])
        hr_t, tr_h = {}, {}
        for h, r, t in allt:
            hr_t.setdefault((int(h), int(r)), set()).add(int(t))
            tr_h.setdefault((int(t), int(r)), set()).add(int(h))
        return hr_t, tr_h

    def build(self, prefix="init.", device="cpu"):
        """The drop-in model holding the fixture's weights under `prefix` and its filters."""
        import pykg2vec_amd as pa
        m = pa.import_model("convkb")(tot_entity=self.E, tot_relation=self.R, device=device, **self.hp)
        m.load_state_dict({k: torch.from_numpy(self.z[prefix + k]) for k in TRAINED})
        with torch.no_grad():
            for j, c in enumerate(m.conv_list):
                c.weight.copy_(torch.from_numpy(self.z["conv.%d.weight" % j]))
                c.bias.copy_(torch.from_numpy(self.z["conv.%d.bias" % j]))
        return m.to(device)


# ---------------------------------------------------------------- the class contract
@pytest.mark.parametrize("name", NAMES)
def test_dropin_class_keeps_reference_contract(name):
    import pykg2vec_amd as pa
    from pykg2vec_amd import integration, pointwise
    from pykg2vec_amd.common import TrainingStrategy
    from pykg2vec_amd.criterion import Criterion
    c = ConvCase(name)
    assert pa.MODEL_MAP["convkb"] == "pointwise.ConvKB" and pa.import_model("convkb") is pointwise.ConvKB
    assert "ConvKB" in integration.POINTWISE
    m = c.build()
    ref_keys = sorted(k[len("init."):] for k in c.z if k.startswith("init."))
    assert ref_keys == sorted(TRAINED)
    assert sorted(m.state_dict().keys()) == ref_keys
    for k in ref_keys:
        assert tuple(m.state_dict()[k].shape) == c.z["init." + k].shape, k
    assert [n for n, _ in m.named_parameters()] == list(TRAINED)
    assert m.parameter_list == [m.ent_embeddings, m.rel_embeddings] and all(hasattr(p, "name") for p in m.parameter_list)
    assert [id(x) for x in m.trainable_tensors()] == [id(p) for _, p in m.named_parameters()]
    # the filters: a plain list of Conv2d(1, F, (3, s)), in no parameter set and no checkpoint
    assert type(m.conv_list) is list and len(m.conv_list) == c.n_filters
    for conv, s in zip(m.conv_list, c.hp["filter_sizes"]):
        assert isinstance(conv, torch.nn.Conv2d) and tuple(conv.weight.shape) == (c.hp["num_filters"], 1, 3, s)
        assert all(conv.weight is not p and conv.bias is not p for p in m.parameters())
    assert not any("conv" in k for k in m.state_dict())
    assert m.model_name == "convkb" and m.training_strategy == TrainingStrategy.POINTWISE_BASED
    assert m.loss is Criterion.pointwise_logistic
    assert m.get_reg(None, None, None) == 0.0
    h, r, t = (torch.from_numpy(x[:5]) for x in c.batch(0)[:3])
    eh, er, et = m.embed(h, r, t)
    assert torch.equal(eh, m.ent_embeddings.weight[h]) and torch.equal(er, m.rel_embeddings.weight[r]) and torch.equal(et, m.ent_embeddings.weight[t])
    for missing in ("tot_entity", "tot_relation", "hidden_size", "num_filters", "filter_sizes", "device"):
        kw = dict(c.hp, tot_entity=c.E, tot_relation=c.R, device="cpu")
        kw.pop(missing)
        with pytest.raises(Exception, match="hyperparameter %s not found!" % missing):
            pointwise.ConvKB(**kw)


def test_xavier_tables_and_packed_filters_follow_writes():
    c = ConvCase("convkb")
    m = c.build()
    fresh = type(m)(tot_entity=c.E, tot_relation=c.R, device="cpu", **c.hp)
    bound = np.sqrt(6.0 / (c.E + c.hp["hidden_size"]))
    w = fresh.ent_embeddings.weight.detach().numpy()
    assert np.abs(w).max() <= bound and np.abs(w).max() > 0.8 * bound          # xavier_uniform_
    cw, cb = m.packed_filters("cpu")
    assert np.array_equal(cw.numpy(), np.concatenate([c.z["conv.%d.weight" % j].reshape(-1) for j in range(c.n_filters)]))
    assert np.array_equal(cb.numpy(), np.concatenate([c.z["conv.%d.bias" % j] for j in range(c.n_filters)]))
    assert m.packed_filters("cpu")[0] is cw                                      # kept ...
    with torch.no_grad():
        m.conv_list[1].weight.mul_(2.0)
    assert m.packed_filters("cpu")[0] is not cw                                  # ... until a filter is written to
    assert torch.equal(m.packed_filters("cpu")[0], torch.cat([x.weight.detach().reshape(-1) for x in m.conv_list]))


def test_forward_is_loud_without_a_gpu():
    from pykg2vec_amd import _lib
    c = ConvCase("convkb")
    m = c.build()
    h, r, t = (torch.from_numpy(x[:4]) for x in c.batch(0)[:3])
    with pytest.raises(_lib.KgeHipError, match="HIP device"):
        m(h, r, t)


# ---------------------------------------------------------------- the math against the frozen reference
@pytest.mark.parametrize("name", NAMES)
def test_affine_form_is_the_convolution_stack(name):
    c = ConvCase(name)
    P = cr.params_from_fixture(c.z)
    h, r, t, _ = c.batch(0)
    assert np.allclose(cr.preds64(P, h, r, t), cr.conv_forward64(P, h, r, t), atol=1e-13, rtol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_reproduces_reference_scores_loss_and_grads(name):
    c = ConvCase(name)
    P = cr.params_from_fixture(c.z)
    h, r, t, y = c.batch(0)
    assert np.allclose(cr.preds64(P, h, r, t), c.z["scores0"], **SCORE_TOL)
    loss, g = cr.step64(P, h, r, t, y)
    assert np.isclose(loss, c.z["loss0"], **SCORE_TOL), (loss, c.z["loss0"])
    assert sorted(k for k in c.z if k.startswith("grad0.")) == sorted("grad0." + k for k in TRAINED)   # the filters get no gradient entry
    for key, got in (("ent_embeddings.weight", g["ent"]), ("rel_embeddings.weight", g["rel"]), ("fc1.weight", g["fc_w"].reshape(1, -1)),
                     ("fc1.bias", np.asarray([g["fc_b"]]))):
        ref = c.z["grad0." + key]
        assert np.allclose(got, ref, **GRAD_TOL), (key, np.abs(got - ref).max())


def test_width_order_fixes_the_column_layout():
    """fc1's columns are laid out in conv_list order: the same filters listed in another order are another model."""
    c = ConvCase("convkb")
    P = cr.params_from_fixture(c.z)
    A, c0 = cr.collapse64(P)
    order = [1, 0, 2]
    Q = cr.make_params(P["ent"], P["rel"], P["fc_w"], P["fc_b"], [c.z["conv.%d.weight" % j] for j in order],
                       [c.z["conv.%d.bias" % j] for j in order])
    B, _ = cr.collapse64(Q)
    assert np.abs(A - B).max() > 1e-3 * np.abs(A).max()


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_reproduces_reference_ranks_and_sweeps(name):
    c = ConvCase(name)
    P = cr.params_from_fixture(c.z, "eval.after.")
    ents = np.arange(c.E)
    hr_t, tr_h = c.filters()
    n = len(c.z["eval.rank_head"])
    assert n == 12
    for i, (h, r, t) in enumerate(c.test[:n]):
        tail = cr.preds64(P, np.full(c.E, h), np.full(c.E, r), ents)
        head = cr.preds64(P, ents, np.full(c.E, r), np.full(c.E, t))
        if i < 4:
            assert np.allclose(tail, c.z["eval.sweeps"][2 * i], **SCORE_TOL) and np.allclose(head, c.z["eval.sweeps"][2 * i + 1], **SCORE_TOL)
        assert cr.rank64(tail, int(t), hr_t[(int(h), int(r))]) == (c.z["eval.rank_tail"][i], c.z["eval.frank_tail"][i])
        assert cr.rank64(head, int(h), tr_h[(int(t), int(r))]) == (c.z["eval.rank_head"][i], c.z["eval.frank_head"][i])
    # the order of the candidates does not depend on the query
    a = cr.preds64(P, np.full(c.E, c.test[0, 0]), np.full(c.E, c.test[0, 1]), ents)
    b = cr.preds64(P, np.full(c.E, c.test[1, 0]), np.full(c.E, c.test[1, 1]), ents)
    assert np.array_equal(np.argsort(a), np.argsort(b))


# ---------------------------------------------------------------- the C boundary
def test_struct_layout_agrees_with_header():
    from pykg2vec_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define KGE_CONVKB_MAX_WIDTHS (\d+)", header).group(1)) == _lib.CONVKB_MAX_WIDTHS == 8
    body = re.search(r"typedef struct kge_convkb_desc \{(.*?)\} kge_convkb_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", x).strip(" *") for x in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [f[0] for f in _lib.ConvKBDesc._fields_]
    # 2 x int64, 3 x int32, 8 x int32, (4 bytes of padding), 10 pointers
    assert ctypes.sizeof(_lib.ConvKBDesc) == 16 + 12 + 32 + 4 + 80
    assert _lib.ConvKBDesc.widths.offset == 28 and _lib.ConvKBDesc.ent.offset == 64 and _lib.ConvKBDesc.g_fc_b.offset == 136
    assert re.search(r"#define KGE_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3


def _good_desc():
    from pykg2vec_amd import _lib
    d = _lib.ConvKBDesc()
    d.tot_entity, d.tot_relation, d.dim, d.num_filters, d.n_widths = 10, 3, 20, 5, 3
    for j, s in enumerate((1, 3, 2)):
        d.widths[j] = s
    for f in ("ent", "rel", "fc_w", "fc_b", "conv_w", "conv_b", "g_ent", "g_rel", "g_fc_w", "g_fc_b"):
        setattr(d, f, 0x1000)    # never dereferenced: every call below is refused before a launch
    return d


def _calls(lib, d, ws, nbytes):
    """name -> thunk of every kge_convkb_* entry point on descriptor d with workspace (ws, nbytes)."""
    p = ctypes.c_void_p(0x1000)
    ref = ctypes.byref(d)
    return {
        "kge_convkb_collapse": lambda: lib.kge_convkb_collapse(ref, p, ws, nbytes, None),
        "kge_convkb_score_forward": lambda: lib.kge_convkb_score_forward(ref, p, p, p, 4, p, ws, nbytes, None),
        "kge_convkb_score_backward": lambda: lib.kge_convkb_score_backward(ref, p, p, p, 4, p, ws, nbytes, None),
        "kge_convkb_train_logistic": lambda: lib.kge_convkb_train_logistic(ref, p, p, p, p, 4, 2, ws, nbytes, p, None),
        "kge_convkb_train_logistic_sampled": lambda: lib.kge_convkb_train_logistic_sampled(ref, p, p, 0, 4, 1, None, None, 0, 1, 0, None, ws,
                                                                                           nbytes, p, None),
        "kge_convkb_eval_ranks": lambda: lib.kge_convkb_eval_ranks(ref, p, 4, None, None, None, None, ws, nbytes, p, None),
        "kge_convkb_sweep_scores_side": lambda: lib.kge_convkb_sweep_scores_side(ref, p, 4, 0, ws, nbytes, p, None),
    }


BAD = {
    "null tables": (lambda d: setattr(d, "conv_w", None), b"null tables"),
    "no widths": (lambda d: setattr(d, "n_widths", 0), b"n_widths must be 1..8"),
    "too many widths": (lambda d: setattr(d, "n_widths", 9), b"n_widths must be 1..8"),
    "zero width": (lambda d: d.widths.__setitem__(1, 0), b"filter width 0"),
    "width beyond dim": (lambda d: d.widths.__setitem__(2, 21), b"filter width 21"),
    "no filters": (lambda d: setattr(d, "num_filters", 0), b"num_filters must be at least 1"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_every_entry_point_refuses_a_bad_descriptor(what):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _good_desc()
    BAD[what][0](d)
    calls = _calls(lib, d, ctypes.c_void_p(0x1000), 1 << 30)
    assert sorted(calls) == sorted(s for s in _lib.EXPORTED_SYMBOLS if s.startswith("kge_convkb_") and not s.endswith("_workspace_bytes"))
    for name, call in calls.items():
        assert call() == -1, name
        msg = lib.kge_last_error()
        assert msg.startswith(name.encode() + b":") and BAD[what][1] in msg, (name, msg)
        assert getattr(lib, name + "_workspace_bytes")(ctypes.byref(d), *([4] if name != "kge_convkb_collapse" else []),
                                                       *([1] if name.endswith("_sampled") else [])) == 0


def test_every_entry_point_refuses_a_small_workspace():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _good_desc()
    for name, call in _calls(lib, d, ctypes.c_void_p(0x1000), 16).items():
        extra = ([4] if name != "kge_convkb_collapse" else []) + ([1] if name.endswith("_sampled") else [])
        need = getattr(lib, name + "_workspace_bytes")(ctypes.byref(d), *extra)
        if name == "kge_convkb_collapse":     # writes straight into `out`: it needs no workspace
            assert need == 0
            continue
        assert need >= (3 * 20 + 1) * 4
        assert call() == -1, name
        msg = lib.kge_last_error()
        assert msg.startswith(name.encode() + b":") and b"workspace too small" in msg, (name, msg)
    for name, call in _calls(lib, d, None, 1 << 30).items():      # a null workspace is too small as well
        if name != "kge_convkb_collapse":
            assert call() == -1 and b"workspace too small" in lib.kge_last_error(), name


def test_gradient_entry_points_refuse_a_forward_descriptor_and_long_bundles():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _good_desc()
    d.g_fc_w = None
    calls = _calls(lib, d, ctypes.c_void_p(0x1000), 1 << 30)
    for name in ("kge_convkb_score_backward", "kge_convkb_train_logistic", "kge_convkb_train_logistic_sampled"):
        assert calls[name]() == -1 and b"null gradient buffers" in lib.kge_last_error(), name
    d = _good_desc()
    p = ctypes.c_void_p(0x1000)
    rc = lib.kge_convkb_train_logistic_sampled(ctypes.byref(d), p, p, 0, 4, 32, None, None, 0, 1, 0, None, p, 1 << 30, p, None)
    assert rc == -1 and b"neg_rate <= 31" in lib.kge_last_error()


def test_trainer_refuses_the_out_of_scope_step_forms():
    """Data-parallel training and the owner-computes / staged forms are not built for ConvKB: refused by name, not fallen through."""
    from pykg2vec_amd.trainer import Trainer
    c = ConvCase("convkb")
    tr = Trainer.__new__(Trainer)
    tr.model = c.build()
    for call in (lambda: tr.own_step_explicit(None, None, None, None), lambda: tr.pull_step_explicit(*[None] * 6),
                 lambda: tr.transx_step_explicit(*[None] * 6), tr._staged_plan):
        with pytest.raises(NotImplementedError, match="ConvKB: .* is not supported"):
            call()
