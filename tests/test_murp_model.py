"""MuRP without a GPU: registration, the reference's state (bit-identical under the recorded seeds), the criterion, the numpy
restatement of tools/murp_reference.py against the frozen reference outputs in tests/golden/ref_murp*.npz, the library's host checks,
the float64 flat buffers and the Trainer's refusals.  The GPU half is tests/test_hip_murp.py, which shares the tolerances below.

Tolerances.  Everything is float64 (eps 2.2e-16) over reductions of k <= 40 terms, so two correct evaluations differ by some 1e-15
relative.  The one amplifier is 1 - x^2 under the square root of arsech at the clamp bound x = 1 - 1e-5, where a relative error of x
grows by 1 / (1 - x^2) = 5e4: 1e-15 * 5e4 = 5e-11.  TOL = 1e-10 of the largest magnitude of the compared array (the restatement
itself lands within 5e-15 of the reference).  The 4-step trajectory at lr = 50 compounds a step's error four times through the
optimiser's lr: TRAJ_TOL = 1e-8."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import murp_reference as mr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("wu", "bs", "bo", "ent_embeddings.weight", "rel_embeddings.weight")
TOL, TRAJ_TOL = 1e-10, 1e-8


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def near(got, want, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= tol * max(float(np.abs(want).max()), 1e-300)))


def worst(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(float(np.abs(want).max()), 1e-300))


def tables(g, prefix):
    return [g[prefix + n] for n in NAMES]


def batch(g, prefix="batch."):
    return [g[prefix + k] for k in "hrty"]


def known_lists(g, h, r, t):
    kn = g["eval.known"]
    return kn[(kn[:, 0] == h) & (kn[:, 1] == r), 2], kn[(kn[:, 2] == t) & (kn[:, 1] == r), 0]


def build(g, device="cpu"):
    import pykg2vec_amd as pa
    seed = int(g["seed"])
    torch.manual_seed(seed)
    np.random.seed(seed)
    return pa.import_model("murp")(tot_entity=int(g["E"]), tot_relation=int(g["R"]), hidden_size=int(g["k"]), lmbda=0.0, device=device)


def cpu_config(optimizer):
    return types.SimpleNamespace(optimizer=optimizer, device="cpu", neg_rate=3, batch_size=8, learning_rate=50.0, tot_entity=97,
                                 tot_relation=7)


# ---------------------------------------------------------------- registration and state
def test_registration():
    import pykg2vec_amd as pa
    from pykg2vec_amd import integration, pointwise
    from pykg2vec_amd.common import TrainingStrategy
    assert pa.import_model("murp") is pointwise.MuRP and pa.import_model("MuRP") is pointwise.MuRP
    assert pa.MODEL_MAP["murp"] == "pointwise.MuRP"
    assert "MuRP" in integration.POINTWISE
    m = build(golden("ref_murp"))
    assert m.training_strategy == TrainingStrategy.POINTWISE_BASED and m.model_name == "murp" and m.kernel_name == "murp"
    assert m.loss.__name__ == "pointwise_bce" and m.get_reg(None, None, None) == 0.0
    assert type(m).rank_order == 0
    with pytest.raises(Exception, match="hyperparameter lmbda not found!"):
        pointwise.MuRP(tot_entity=5, tot_relation=2, hidden_size=4, device="cpu")


def test_initial_state_is_the_references_bit_for_bit():
    g = golden("ref_murp")
    m = build(g)
    sd = m.state_dict()
    assert tuple(sd.keys()) == NAMES == tuple(n for n, _ in m.named_parameters())
    for n in NAMES:
        assert sd[n].dtype == torch.float64 and tuple(sd[n].shape) == g["init." + n].shape
        assert np.array_equal(sd[n].numpy(), g["init." + n]), n
    assert [p.name for p in m.parameter_list] == ["ent_embedding", "rel_embedding"]
    assert m.ent_embeddings.padding_idx == 0 and m.rel_embeddings.padding_idx == 0
    assert [t.data_ptr() for t in m.trainable_tensors()] == [sd[n].data_ptr() for n in NAMES]
    m.load_state_dict({n: torch.from_numpy(g["live." + n]) for n in NAMES})      # a reference checkpoint loads as it is


def test_criterion_pointwise_bce():
    from pykg2vec_amd.criterion import Criterion
    g = golden("ref_murp")
    loss = Criterion.pointwise_bce(torch.from_numpy(g["step.preds"]), torch.from_numpy(g["batch.y"]).double())
    assert abs(loss.item() - float(g["step.loss"])) <= np.spacing(float(g["step.loss"]))


# ---------------------------------------------------------------- the restatement against the live reference's recorded outputs
@pytest.mark.parametrize("name", ["ref_murp", "ref_murp_k40"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_restatement_step_matches_reference(name, dtype):
    g = golden(name)
    tabs = tables(g, "live.")
    preds, loss, grads = mr.train_bce(tabs, *batch(g), dtype=dtype)
    print("preds", worst(preds, g["step.preds"]), "grads", [worst(a, g["step.grad." + n]) for a, n in zip(grads, NAMES)])
    assert near(preds, g["step.preds"]) and near(loss, g["step.loss"])
    for a, n in zip(grads, NAMES):
        assert near(a, g["step.grad." + n]), (n, worst(a, g["step.grad." + n]))
    ref_grads = [g["step.grad." + n] for n in NAMES]
    for mode, riemannian in (("riemannian", True), ("sgd", False)):
        for a, n in zip(mr.rsgd_step(tabs, ref_grads, float(g["lr"]), riemannian, dtype), NAMES):
            assert near(a, g["step.%s.%s" % (mode, n)]), (mode, n)


def test_reference_gradient_conventions_hold_in_the_golden():
    g = golden("ref_murp")
    h, r, t, _ = batch(g)
    sat = g["batch.saturated"]
    assert sat.any() and not sat.all() and (h == 0).any() and (r == 0).any() and (t == 0).any()
    assert not g["step.grad.ent_embeddings.weight"][0].any() and not g["step.grad.rel_embeddings.weight"][0].any()   # padding_idx
    assert g["step.grad.wu"][0].any() and g["step.grad.bs"][0] != 0 and g["step.grad.bo"][0] != 0
    # rows the optimiser's gradient is zero for come out bit-identical
    untouched = ~g["step.grad.ent_embeddings.weight"].any(1)
    assert untouched.any()
    assert np.array_equal(g["step.riemannian.ent_embeddings.weight"][untouched], g["live.ent_embeddings.weight"][untouched])
    # a batch of saturated rows alone: bs and bo get their gradient, wu / ent / rel exact zeros
    grads = mr.backward(tables(g, "live."), h[sat], r[sat], t[sat], np.ones(int(sat.sum())))
    assert not grads[0].any() and not grads[3].any() and not grads[4].any() and grads[1].any() and grads[2].any()


def test_restatement_zero_row_is_finite():
    g = golden("ref_murp")
    tabs = [a.copy() for a in tables(g, "live.")]
    tabs[3][9] = 0.0
    tabs[4][2] = 0.0
    h, r, t = np.array([9, 4, 9]), np.array([2, 2, 1]), np.array([4, 9, 9])
    grads = mr.backward(tabs, h, r, t, np.ones(3))
    assert all(np.isfinite(a).all() for a in grads) and np.isfinite(mr.forward(tabs, h, r, t)).all()


def test_restatement_trajectory_matches_reference():
    g = golden("ref_murp")
    tabs = tables(g, "init.")
    for i in range(4):
        _, loss, grads = mr.train_bce(tabs, *batch(g, "traj.batch%d." % i))
        assert near(loss, g["traj.loss"][i], TRAJ_TOL)
        tabs = mr.rsgd_step(tabs, grads, float(g["lr"]))
    for a, n in zip(tabs, NAMES):
        assert near(a, g["traj.after." + n], TRAJ_TOL), (n, worst(a, g["traj.after." + n]))


def test_restatement_sweeps_reproduce_the_reference_lists_and_ranks():
    """The contracted sweeps give the reference's predict_*_rank lists; the list position of the true entity is the rank_order = 0
    count, and the reference MetricCalculator's ranks (it walks a list from its end) are the rank_order = 1 counts."""
    g = golden("ref_murp")
    tabs = tables(g, "live.")
    E = int(g["E"])
    ents = np.arange(E)
    for i, (h, r, t) in enumerate(g["eval.queries"]):
        st, sh = mr.sweep_tail(tabs, h, r), mr.sweep_head(tabs, r, t)
        assert near(st, mr.forward(tabs, np.full(E, h), np.full(E, r), ents)) and near(sh, mr.forward(tabs, ents, np.full(E, r), np.full(E, t)))
        assert np.array_equal(np.argsort(st, kind="stable"), g["eval.tail_list"][i])
        assert np.array_equal(np.argsort(sh, kind="stable"), g["eval.head_list"][i])
        kt, kh = known_lists(g, h, r, t)
        assert mr.ranks(st, t, kt, 0)[::2] == (g["eval.pos_tail"][i], 0) and mr.ranks(sh, h, kh, 0)[::2] == (g["eval.pos_head"][i], 0)
        assert mr.ranks(st, t, kt, 1)[:2] == (g["eval.rank_tail"][i], g["eval.frank_tail"][i])
        assert mr.ranks(sh, h, kh, 1)[:2] == (g["eval.rank_head"][i], g["eval.frank_head"][i])


def test_restatement_tie_band():
    """Saturated candidates tie bit for bit (bs = bo = 0): the reference's list position lies inside the count's tie band."""
    g = golden("ref_murp_ties")
    tabs = tables(g, "live.")
    tied = 0
    for i, (h, r, t) in enumerate(g["eval.queries"]):
        for s, true, pos in ((mr.sweep_tail(tabs, h, r), t, g["eval.pos_tail"][i]), (mr.sweep_head(tabs, r, t), h, g["eval.pos_head"][i])):
            rank, _, ties = mr.ranks(s, true, (), 0)
            assert rank <= pos <= rank + ties
            tied += ties
    assert tied > 0


# ---------------------------------------------------------------- library host checks, bindings, ops
def test_library_refuses_bad_descriptors_without_gpu():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    d = _lib.MurpDesc()
    d.tot_entity, d.tot_relation, d.dim = 10, 3, 8
    assert ctypes.sizeof(_lib.MurpDesc) == 8 + 8 + 4 + 4 + 8 * 10 and _lib.MurpDesc.tables.offset == 24
    assert lib.kge_murp_score_forward(ctypes.byref(d), None, None, None, 4, None, None) != 0
    assert b"null tables" in lib.kge_last_error()
    buf = (ctypes.c_double * 128)()
    for i in range(5):
        d.tables[i] = ctypes.addressof(buf)
    for dim in (0, 2049):
        d.dim = dim
        assert lib.kge_murp_score_forward(ctypes.byref(d), None, None, None, 0, None, None) != 0
        assert b"dim must be 1..2048" in lib.kge_last_error()
    d.dim, d.rank_order = 8, 2
    assert lib.kge_murp_eval_ranks_workspace_bytes(ctypes.byref(d), 4) == 0 and b"rank_order" in lib.kge_last_error()
    d.rank_order = 0
    assert lib.kge_murp_train_bce(ctypes.byref(d), None, None, None, None, 0, ctypes.addressof(buf), None) != 0
    assert b"null gradient buffers" in lib.kge_last_error()
    need = lib.kge_murp_eval_ranks_workspace_bytes(ctypes.byref(d), 4)
    assert need > 0 and need % 256 == 0
    trip = (ctypes.c_int64 * 12)()
    ranks = (ctypes.c_int32 * 16)()
    assert lib.kge_murp_eval_ranks(ctypes.byref(d), ctypes.addressof(trip), 4, None, None, None, None, ctypes.addressof(buf), need - 1,
                                   ctypes.addressof(ranks), None, None) != 0
    assert b"workspace" in lib.kge_last_error()


def test_descriptor_builder_and_op_refuse_cpu_tensors():
    from pykg2vec_amd import _lib
    m = build(golden("ref_murp"))
    with pytest.raises(_lib.KgeHipError, match="HIP device"):
        m.make_desc()
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.KgeHipError, match="kge::murp_score"):
        m(ids, ids, ids)


# ---------------------------------------------------------------- flat buffers and the Trainer's choices
def test_flat_state_is_float64_for_murp_and_float32_by_default():
    import pykg2vec_amd as pa
    from pykg2vec_amd.state import FlatState
    g = golden("ref_murp")
    m = build(g)
    flat = FlatState(m, "riemannian", backend=None, dtype=torch.float64)
    assert flat.param.dtype == flat.grad.dtype == torch.float64 and flat.state1 is None and flat.state2 is None
    assert all(o % 4 == 0 for o in flat.offsets) and len(flat.views) == 5
    sd = m.state_dict()
    for n in NAMES:     # re-homed, still the reference's keys, dtypes and values
        assert sd[n].dtype == torch.float64 and np.array_equal(sd[n].numpy(), g["init." + n])
    flat.param.zero_()
    assert not m.wu.any() and not m.ent_embeddings.weight.any()
    d = pa.import_model("distmult")(tot_entity=9, tot_relation=3, hidden_size=4, lmbda=0.0)
    assert FlatState(d, "adam", backend=None).param.dtype == torch.float32


@pytest.mark.parametrize("opt", ["adam", "adagrad", "rms"])
def test_trainer_refuses_other_optimizers(opt):
    from pykg2vec_amd.trainer import Trainer
    tr = Trainer(build(golden("ref_murp")), cpu_config(opt))
    with pytest.raises(NotImplementedError, match=r"MuRP: the %s optimizer is not supported \(riemannian and sgd only\)" % opt):
        tr.build_model()


def test_riemannian_stays_refused_for_other_models():
    import pykg2vec_amd as pa
    from pykg2vec_amd.trainer import Trainer
    d = pa.import_model("distmult")(tot_entity=9, tot_relation=3, hidden_size=4, lmbda=0.0)
    with pytest.raises(NotImplementedError, match="No support for riemannian optimizer"):
        Trainer(d, cpu_config("riemannian")).build_model()


def test_trainer_single_gpu_refusals():
    from pykg2vec_amd.trainer import Trainer
    tr = Trainer(build(golden("ref_murp")), cpu_config("riemannian"), use_graph=True)
    with pytest.raises(NotImplementedError, match=r"MuRP: hipGraph capture of the step is not supported \(single-GPU fused step only\)"):
        tr.build_model()
    tr = Trainer(build(golden("ref_murp")), cpu_config("riemannian"))
    tr.switches["pw_pull"] = True
    with pytest.raises(NotImplementedError, match=r"MuRP: the owner-computes step \(KGE_PW_PULL=1\) is not supported"):
        tr.build_model()
    tr = Trainer(build(golden("ref_murp")), cpu_config("riemannian"))
    for entry, n_args in (("pull_step_explicit", 6), ("own_step_explicit", 4), ("transx_step_explicit", 6)):
        with pytest.raises(NotImplementedError, match="MuRP: the owner-computes step is not supported"):
            getattr(tr, entry)(*([None] * n_args))
    with pytest.raises(NotImplementedError, match="MuRP: the staged step is not supported"):
        tr._staged_plan()
    assert tr._fused_pointwise_ok() is False and tr.step_path() == "murp"
