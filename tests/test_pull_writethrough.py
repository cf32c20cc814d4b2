"""Write-through row stores of the owner-computes TransE step (csrc/kge_pull_device.h: store16_wt; switches KGE_WT_S1, KGE_WT_S2,
KGE_WT_TAB, KGE_WT_HAT for the four streams of pull_finish_row, KGE_WT_EVAL for k_pull_eval's records and codes).  The flavour of a
store changes WHEN its bytes leave the XCD's L2, never the bytes: three consecutive steps through the Trainer -- a row written
through in step k is read by another XCD's owner in step k + 1 -- must leave both tables, both Adam moments, the normalised rows,
the norms and the loss buffer identical to the run with every switch off, for the combination that ships as default and for all
switches on."""
import numpy as np
import pytest
import torch

import kge_oracle as ko

pytestmark = pytest.mark.gpu

SWITCHES = ("KGE_WT_S1", "KGE_WT_S2", "KGE_WT_TAB", "KGE_WT_HAT", "KGE_WT_EVAL")
ALL_OFF = dict.fromkeys(SWITCHES, "0")
COMBOS = {
    "default": {},                                # whatever csrc/kge_pull.hip: write_through_mask() ships
    "all_on": dict.fromkeys(SWITCHES, "1"),
}
#        d    E   R    B  two-phase
SHAPES = {
    "d100": (100, 300, 7, 512, "1"),             # 25 of 32 lanes store; relations with > 32 pairs: workgroup-local segments, k_pull_finish
    "d128": (128, 300, 7, 512, "1"),             # every lane stores
    "d36": (36, 300, 7, 512, "1"),               # a short row
    "overflow": (100, 8, 2, 256, "1"),           # an entity drawn by more than 16 pairs: the overflow walk
    "one_phase": (100, 300, 7, 128, "0"),        # the one-phase step shares pull_finish_row
}
_reference = {}


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def _three_steps(hip, monkeypatch, shape, env):
    from pykg2vec_amd.trainer import Trainer
    d, E, R, B, two_phase = SHAPES[shape]
    rng = np.random.default_rng(99)
    n = 3 * B + 1
    # head and tail of a training triple have the same parity: every (h, r, .) and (., r, t) keeps E / 2 corruptions that are no
    # training triple, so the filtered sampler always finds one (at E = 8, R = 2 unrestricted triples would cover all 128 combinations)
    heads = rng.integers(E, size=n)
    train = np.stack([heads, rng.integers(R, size=n), (rng.integers(E, size=n) & ~1) | (heads & 1)], 1)
    P = ko.init_params("transe", rng, tot_entity=E, tot_relation=R, hidden_size=d)
    hp = dict(hidden_size=d, l1_flag=True, margin=1.0)
    cfg = hip.make_config(E, R, hp, train[:1], train[:4], train[:4], optimizer="adam", lr=0.01, batch_size=B)
    cfg.knowledge_graph.cache["triplets_train"] = train
    cfg.tot_train_triples = len(train)
    monkeypatch.setenv("KGE_PULL", "1")
    monkeypatch.setenv("KGE_PULL_DIR", two_phase)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = Trainer(hip.model_from_params("transe", P, hp, E, R), cfg, use_graph=False)
    tr.build_model()
    tr.generator = tr._new_generator()
    assert tr._pull_ok() and tr._pull_two_phase() == (two_phase == "1")
    tr.train_model_epoch(0)
    assert tr.flat.step == 3
    ps = tr._pull
    torch.cuda.synchronize()
    out = {"tables": tr.flat.param, "other_half": ps.alt, "moment1": tr.flat.state1, "moment2": tr.flat.state2, "loss": tr.loss_buf}
    for half in (0, 1):
        out["hat%d" % half] = ps.hat_all[half]
        out["norms%d" % half] = ps.norms[half]
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_write_through_stores_change_no_byte(hip, monkeypatch, shape, combo):
    if shape not in _reference:
        _reference[shape] = _three_steps(hip, monkeypatch, shape, ALL_OFF)
    ref = _reference[shape]
    assert float(ref["moment2"].abs().max()) > 0 and float(ref["loss"].double().abs().sum()) > 0   # (the steps did run)
    got = _three_steps(hip, monkeypatch, shape, COMBOS[combo])
    for k in ref:
        assert torch.equal(ref[k], got[k]), (shape, combo, k)
