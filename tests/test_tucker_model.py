"""TuckER without a GPU: the drop-in class keeps the reference's construction contract, the float64 restatement
(tools/tucker_reference.py) reproduces the reference's float64 outputs frozen in tests/golden/ref_tucker{,_ls}.npz, the Philox mask
restatement has the right keep rate, every refusal raises with its sentence, and the ctypes struct agrees with the header."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import tucker_reference as tr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["tucker", "tucker_ls"]
TABLES = ("ent_embeddings.weight", "rel_embeddings.weight", "W.weight")
PARAMS = dict(tot_entity=70, tot_relation=5, ent_hidden_size=20, rel_hidden_size=12, lmbda=0.0, input_dropout=0.3, hidden_dropout1=0.4,
              hidden_dropout2=0.5)


def fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)))
    z["ls"] = None if z["label_smoothing"] < 0 else float(z["label_smoothing"])
    return z


def tables(z):
    return {k: z[k].astype(np.float64) for k in TABLES}


def build(**over):
    from pykg2vec_amd.projection import TuckER
    kw = dict(PARAMS)
    kw.update(over)
    return TuckER(**kw)


@pytest.mark.parametrize("missing", sorted(PARAMS))
def test_constructor_names_the_missing_parameter(missing):
    from pykg2vec_amd.projection import TuckER
    kw = {k: v for k, v in PARAMS.items() if k != missing}
    with pytest.raises(Exception, match=missing):
        TuckER(**kw)


def test_class_contract():
    from pykg2vec_amd import TrainingStrategy, import_model
    from pykg2vec_amd.criterion import Criterion
    from pykg2vec_amd.kgmeta import ProjectionModel
    m = build()
    assert import_model("tucker") is type(m) and isinstance(m, ProjectionModel)
    assert m.model_name == "tucker" and m.training_strategy == TrainingStrategy.PROJECTION_BASED
    assert m.loss is Criterion.multi_class_bce and m.get_reg(None, None, None) == 0.0
    z = fixture("tucker")
    sd = m.state_dict()
    assert sorted(sd) == sorted(TABLES)
    assert [tuple(sd[k].shape) for k in TABLES] == [z[k].shape for k in TABLES] == [(70, 20), (5, 12), (12, 400)]
    m.load_state_dict({k: torch.from_numpy(z[k].astype(np.float32)) for k in TABLES}, strict=True)   # a reference state dict
    assert [t.shape for t in m.trainable_tensors()] == [sd[k].shape for k in TABLES]
    m.eval()
    assert not m.training
    m.train()
    assert m.training
    with pytest.raises(AssertionError, match="Unknown forward direction"):
        m.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), direction="sideways")


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_float64(name):
    z = fixture(name)
    loss, g, pt, ph = tr.step(tables(z), z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"])
    assert abs(loss - z["loss"]) <= 1e-9 * abs(z["loss"])
    assert np.allclose(pt, z["pred_tails"], rtol=1e-9, atol=0) and np.allclose(ph, z["pred_heads"], rtol=1e-9, atol=0)
    for k in TABLES:
        assert np.abs(g[k] - z["grad." + k]).max() <= 1e-9 * np.abs(z["grad." + k]).max(), k
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    ranks, gap = tr.ranks(tables(z), z["test"], known)
    assert np.array_equal(ranks, z["ranks"]) and gap > 1e-6


@pytest.mark.parametrize("site,p", [(0, 0.3), (1, 0.4), (2, 0.5)])
def test_mask_keep_rate(site, p):
    n = 1000 * 1000
    m = tr.mask(site, 1000, 1000, p, seed=12345, offset=7)
    kept = int((m != 0).sum())
    q = 1.0 - float(np.float32(p))
    assert abs(kept - n * q) <= 4.0 * np.sqrt(n * q * (1 - q)), (kept, n * q)
    assert set(np.unique(m)) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}


def test_masks_differ_between_sites_rows_and_offsets():
    a = tr.mask(0, 8, 64, 0.5, seed=3)
    assert not np.array_equal(a, tr.mask(2, 8, 64, 0.5, seed=3))
    assert not np.array_equal(a, tr.mask(0, 8, 64, 0.5, seed=4))
    assert not np.array_equal(a, tr.mask(0, 8, 64, 0.5, seed=3, offset=1))
    assert len({row.tobytes() for row in a}) == 8
    assert np.array_equal(tr.mask(1, 3, 16, 0.0), np.ones((3, 16)))


# ---------------------------------------------------------------- refusals
SWITCHES = ("KGE_PULL", "KGE_PW_PULL", "KGE_STAGED", "KGE_TRANSX_OWN", "KGE_GRAPH_MULTI", "KGE_DP_SPARSE", "KGE_DP_ALLREDUCE")

def config(**kw):
    base = dict(optimizer="adam", neg_rate=0, device="cpu", batch_size=8, learning_rate=0.01, seed=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("what,kw,env", [
    ("riemannian optimizer", dict(optimizer="riemannian"), {}),
    ("neg_rate > 0", dict(neg_rate=1), {}),
    (r"owner-computes step \(KGE_PW_PULL=1\)", {}, {"KGE_PW_PULL": "1"}),
    (r"staged step \(KGE_STAGED=1\)", {}, {"KGE_STAGED": "1"}),
])
def test_trainer_refuses(monkeypatch, what, kw, env):
    from pykg2vec_amd.trainer import Trainer
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(NotImplementedError, match="TuckER: .*%s.* is not supported on the projection path" % what):
        Trainer(build(), config(**kw)).build_model()


def test_path_switches_of_other_models_do_not_refuse(monkeypatch):
    """KGE_PULL / KGE_TRANSX_OWN choose between the step paths of the translation models; other tests of this suite leave them set in
    the process environment.  A projection model never enters those paths, so they are no request about it: past the refusals,
    build_model goes on to the flat buffers, which need the HIP device."""
    from pykg2vec_amd.trainer import Trainer
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KGE_PULL", "1")
    monkeypatch.setenv("KGE_TRANSX_OWN", "1")
    t = Trainer(build(), config())
    t._refuse_projection()


def test_trainer_refuses_graph_capture_and_data_parallel(monkeypatch):
    from pykg2vec_amd.trainer import Trainer
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(NotImplementedError, match="hipGraph capture"):
        Trainer(build(), config(), use_graph=True).build_model()
    t = Trainer(build(), config())
    t.distributed = True
    with pytest.raises(NotImplementedError, match="data-parallel training"):
        t.build_model()


def test_generator_refuses_negatives():
    from pykg2vec_amd.generator import Generator
    with pytest.raises(NotImplementedError, match="neg_rate > 0 is not supported"):
        Generator(build(), config(neg_rate=2))


# ---------------------------------------------------------------- C ABI
def test_struct_layout_agrees_with_header():
    from pykg2vec_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    body = re.search(r"typedef struct kge_tucker_desc \{(.*?)\} kge_tucker_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [x.strip(" *") for x in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    assert names == [f[0] for f in _lib.TuckerDesc._fields_]
    # 2 x int64, 2 x int32, 3 x float, int32, 2 x uint64, 6 pointers: no padding
    assert ctypes.sizeof(_lib.TuckerDesc) == 16 + 8 + 12 + 4 + 16 + 48
    assert _lib.TuckerDesc.seed.offset == 40 and _lib.TuckerDesc.ent.offset == 56 and _lib.TuckerDesc.g_W.offset == 96
    assert re.search(r"#define KGE_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3


SYMBOLS = ["kge_tucker_saved_floats", "kge_tucker_body_forward", "kge_tucker_body_backward", "kge_tucker_train_bce", "kge_tucker_eval_ranks"] + \
          ["kge_tucker_%s_workspace_bytes" % s for s in ("body_forward", "body_backward", "train_bce", "eval_ranks")]


def test_symbols_are_exported():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


def _desc():
    from pykg2vec_amd import _lib
    d = _lib.TuckerDesc()
    d.tot_entity, d.tot_relation, d.d1, d.d2 = 10, 3, 20, 12
    for f in ("ent", "rel", "W", "g_ent", "g_rel", "g_W"):
        setattr(d, f, 0x1000)    # never dereferenced: every call below is refused before a launch
    return d


@pytest.mark.parametrize("field,value,msg", [("ent", None, "null tables"), ("d1", 0, "must be positive"), ("d1", 40000, "d1 = 40000"),
                                             ("hidden_dropout1", 1.0, "dropout rate 1"), ("input_dropout", -0.1, "dropout rate 0"),
                                             ("offset", 1 << 62, "offset"), ("g_W", None, "null gradient buffers")])
def test_entry_points_refuse_bad_descriptors(field, value, msg):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    setattr(d, field, value)
    p = ctypes.c_void_p(0x1000)
    rc = lib.kge_tucker_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, 1 << 30, p, None)
    assert rc != 0 and msg in lib.kge_last_error().decode() and "kge_tucker_train_bce" in lib.kge_last_error().decode()
    if field != "g_W":
        assert lib.kge_tucker_body_forward_workspace_bytes(ctypes.byref(d), 4) == 0
        assert lib.kge_tucker_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, 1 << 30, p, None, None) != 0


def test_entry_points_refuse_small_workspaces():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _desc()
    p = ctypes.c_void_p(0x1000)
    assert lib.kge_tucker_body_forward_workspace_bytes(ctypes.byref(d), 4) > 0
    assert lib.kge_tucker_body_forward(ctypes.byref(d), p, p, 4, p, p, p, 16, None) != 0
    assert "workspace too small" in lib.kge_last_error().decode()
    assert lib.kge_tucker_body_backward(ctypes.byref(d), p, p, 4, p, p, None, 0, None) != 0
    assert lib.kge_tucker_train_bce(ctypes.byref(d), p, p, p, 4, p, p, 1, p, p, 1, -1.0, p, 16, p, None) != 0
    assert lib.kge_tucker_eval_ranks(ctypes.byref(d), p, 4, None, None, None, None, p, 16, p, None, None) != 0
    assert "kge_tucker_eval_ranks: workspace too small" in lib.kge_last_error().decode()
