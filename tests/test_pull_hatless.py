"""Hat-less two-phase owner-computes step (csrc/kge_pull.hip: k_pull_eval_nohat + k_pull_step_nohat, switch KGE_PULL_HATLESS): phase 1
gathers the table rows and scales them by 1 / max(norm, eps) itself, the owners write no normalised rows.  The scaled row is the hat row
bit for bit, so three consecutive steps through the Trainer must leave both tables, the other half of the double buffer, both Adam
moments, the norms and the loss buffer identical to the run with the switch off (the hat tables themselves are no longer maintained and
are not compared).  One more case proves that hats left stale by hat-less steps are rebuilt before a launch reads them."""
import numpy as np
import pytest
import torch

import kge_oracle as ko

pytestmark = pytest.mark.gpu

#        model     d    E   R    B  zero rows
SHAPES = {
    "d100": ("transe", 100, 300, 7, 512, False),        # 25 of 32 lanes load; relations with > 32 pairs: workgroup-local segments, k_pull_finish
    "d128": ("transe", 128, 300, 7, 512, False),        # every lane loads
    "d36": ("transe", 36, 300, 7, 512, False),          # a short row
    "overflow": ("transe", 100, 8, 2, 256, False),      # an entity drawn by more than 16 pairs: the overflow walk
    "zero_row": ("transe", 100, 300, 7, 512, True),     # an entity and a relation row of zeros: norm <= eps, the fmaxf branch
    "transm": ("transm", 100, 300, 7, 512, False),      # theta != NULL: the float visit path
}
_reference = {}


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def _trainer(hip, monkeypatch, shape, hatless, n_steps):
    from pykg2vec_amd.trainer import Trainer
    model, d, E, R, B, zero_rows = SHAPES[shape]
    rng = np.random.default_rng(99)
    n = n_steps * B + 1
    # head and tail of a training triple have the same parity: every (h, r, .) and (., r, t) keeps E / 2 corruptions that are no
    # training triple, so the filtered sampler always finds one (at E = 8, R = 2 unrestricted triples would cover all 128 combinations)
    heads = rng.integers(E, size=n)
    train = np.stack([heads, rng.integers(R, size=n), (rng.integers(E, size=n) & ~1) | (heads & 1)], 1)
    P = ko.init_params(model, rng, tot_entity=E, tot_relation=R, hidden_size=d)
    if zero_rows:   # rows the first batch visits in every role
        P["ent_embeddings"][train[0, 0]] = 0.0
        P["ent_embeddings"][train[1, 2]] = 0.0
        P["rel_embeddings"][train[0, 1]] = 0.0
    hp = dict(hidden_size=d, l1_flag=True, margin=1.0)
    cfg = hip.make_config(E, R, hp, train[:1], train[:4], train[:4], optimizer="adam", lr=0.01, batch_size=B)
    cfg.knowledge_graph.cache["triplets_train"] = train
    cfg.tot_train_triples = len(train)
    monkeypatch.setenv("KGE_PULL", "1")
    monkeypatch.setenv("KGE_PULL_DIR", "1")
    monkeypatch.setenv("KGE_PULL_HATLESS", hatless)
    tr = Trainer(hip.model_from_params(model, P, hp, E, R, train=train), cfg, use_graph=False)
    tr.build_model()
    tr.generator = tr._new_generator()
    assert tr._pull_ok() and tr._pull_two_phase()
    return tr


def _state(tr):
    ps = tr._pull
    torch.cuda.synchronize()
    out = {"tables": tr.flat.param, "other_half": ps.alt, "moment1": tr.flat.state1, "moment2": tr.flat.state2, "loss": tr.loss_buf}
    for half in (0, 1):
        out["norms%d" % half] = ps.norms[half]
    return {k: v.detach().clone() for k, v in out.items()}


def _three_steps(hip, monkeypatch, shape, hatless):
    from pykg2vec_amd import kernels as K
    tr = _trainer(hip, monkeypatch, shape, hatless, 3)
    assert K.pull_hatless() == (hatless == "1")
    tr.train_model_epoch(0)
    assert tr.flat.step == 3 and tr._pull.hats_stale == (hatless == "1")
    return _state(tr)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_hatless_steps_change_no_byte(hip, monkeypatch, shape):
    ref = _reference[shape] = _three_steps(hip, monkeypatch, shape, "0")
    assert float(ref["moment2"].abs().max()) > 0 and float(ref["loss"].double().abs().sum()) > 0   # (the steps did run)
    got = _three_steps(hip, monkeypatch, shape, "1")
    for k in ref:
        assert torch.equal(ref[k], got[k]), (shape, k)


def _three_then_one_phase(hip, monkeypatch, hatless):
    """Three two-phase steps, then a one-phase step -- whose owners gather hat rows -- on the same state, inside one epoch."""
    tr = _trainer(hip, monkeypatch, "d100", hatless, 4)
    tr.generator.start_one_epoch(4)
    tr.loss_buf.zero_()
    ps = tr._pull_state()[0]
    ps.sync_in()
    tr.step_next_batches(3)
    assert ps.hats_stale == (hatless == "1") and ps.cur == 1
    tr.switches["pull_dir"] = False            # KGE_PULL_DIR=0 from here on
    tr.step_next_batches(1)
    assert tr._pull is ps and not ps.plan_two_phase and not ps.hats_stale and tr.flat.step == 4
    tr.sync_model()
    out = _state(tr)
    out["hat"] = ps.hat_all[0].detach().clone()     # the one-phase step wrote them again
    return out


def test_stale_hats_are_rebuilt_before_a_one_phase_step(hip, monkeypatch):
    ref = _three_then_one_phase(hip, monkeypatch, "0")
    assert float(ref["hat"].abs().max()) > 0
    got = _three_then_one_phase(hip, monkeypatch, "1")
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
