"""Hat-less two-phase step with STORED inverse norms (csrc/kge_pull.hip): the owners store 1 / max(norm, eps) next to each norm,
k_pull_eval_nohat loads the eight scales of a lane group instead of loading norms and dividing (one ds_bpermute per row), and all four
evaluation kernels take the direction codes from the ordering of the residual against zero instead of clamp(x * 2^100, -1, 1).  None of
this may move a byte: after each of three two-phase Adam steps the tables, the other half of the double buffer, both moments, both norm
buffers, the pairs' records and their direction codes must equal those of the same tree with KGE_PULL_HATLESS=0 (the hat-carrying arm,
which the round-30 tests hold to the parent bit for bit).

Shapes are the smallest at which each part can still go wrong (the index geometry is the Trainer's own, from kge_pull_index_geometry):
more lane groups than pairs (the dead-pair clamp feeds the last pair's ids to the scale hand-off; one wave holds a live and a dead
group), an odd pair count at d = 100 (25 of 32 lanes live), d = 132 (two float4s per lane), a zero row (stored inverse = 1 / eps),
residual elements that are exactly +0 and -0 (code 0), float32 subnormals (the sign test against the 2^100 form -- judged by the
reference arm, not by a formula here), TransM (the float visit path reads the same records), and a mixed run that pins the validity of
the stored inverse norms across one-phase steps, fresh_hats() and sync_in()."""
import numpy as np
import pytest
import torch

import kge_oracle as ko

pytestmark = pytest.mark.gpu

#          model     E   R   d    B  margin  special
SHAPES = {
    "dead_groups": ("transe", 5, 2, 4, 3, 1.0, None),
    "odd_pairs_d100": ("transe", 40, 3, 100, 17, 1.0, None),
    "d132": ("transe", 33, 2, 132, 9, 1.0, None),
    "zero_row": ("transe", 40, 3, 100, 17, 1.0, "zero_row"),
    "signed_zeros": ("transe", 40, 3, 100, 17, 50.0, "signed_zeros"),   # (margin: the hinge of pair 0 is active, so its codes are written)
    "subnormals": ("transe", 40, 3, 100, 17, 50.0, "subnormals"),
    "transm": ("transm", 40, 3, 100, 17, 1.0, None),
}
ZERO_AT, NEGZERO_AT = (0, 5, 33), (2, 7, 64)   # elements of pair 0's positive residual that are exactly +0 / -0 in "signed_zeros"


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def _trainer(hip, monkeypatch, shape, hatless, n_steps):
    from pykg2vec_amd.trainer import Trainer
    model, E, R, d, B, margin, special = SHAPES[shape]
    rng = np.random.default_rng(31)
    n = n_steps * B + 1
    # head and tail of a training triple have the same parity: every (h, r, .) and (., r, t) keeps corruptions that are no training
    # triple, so the filtered sampler always finds one
    heads = rng.integers(E, size=n)
    tails = 2 * rng.integers((E - (heads & 1) + 1) // 2) + (heads & 1)
    train = np.stack([heads, rng.integers(R, size=n), tails], 1)
    P = ko.init_params(model, rng, tot_entity=E, tot_relation=R, hidden_size=d)
    hp = dict(hidden_size=d, l1_flag=True, margin=margin)
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


def _shape_one_pair(tr, shape):
    """The special cases: reshape the three rows of one pair of the first batch (the first with h != t) on the device, before the norms
    are derived.  Returns the pair's index in the batch."""
    d, special = SHAPES[shape][3], SHAPES[shape][6]
    ps, idx = tr._pull_state()
    pairs = idx.batch(0)[0].cpu().numpy()
    q = int(np.flatnonzero(pairs[:, 0] != pairs[:, 2])[0])
    h, r, t = (int(x) for x in pairs[q, :3])
    ent, rel = ps.tables[0]
    if special == "zero_row":
        ent[h] = 0.0
    elif special == "signed_zeros":   # h^ == t^ and r^ == 0 -> +0; h^ = -0, r^ = -0, t^ = +0 -> (-0 + -0) - (+0) = -0
        ent[t] = ent[h]
        rel[r, list(ZERO_AT)] = 0.0
        ent[h, list(NEGZERO_AT)] = -0.0
        ent[t, list(NEGZERO_AT)] = 0.0
        rel[r, list(NEGZERO_AT)] = -0.0
    elif special == "subnormals":     # half of each row of the pair about 1e-41: subnormal before and after the division by a norm of ~1
        rng = np.random.default_rng(41)
        for row in (ent[h], rel[r], ent[t]):
            row[:d // 2] = torch.from_numpy((rng.choice([-3, -2, -1, 1, 2, 3], size=d // 2) * 1e-41).astype(np.float32)).to(row.device)
        assert 0 < float(ent[h, :d // 2].abs().max()) < float(np.finfo(np.float32).tiny)
    ps.sync_in()
    return q


def _state(tr, out, tag):
    ps = tr._pull
    torch.cuda.synchronize()
    cur = {"tables": tr.flat.param, "other_half": ps.alt, "moment1": tr.flat.state1, "moment2": tr.flat.state2,
           "norms0": ps.norms[0], "norms1": ps.norms[1], "recs": ps.direction.recs, "codes": ps.direction.codes}
    out.update({"%s/%s" % (tag, k): v.detach().clone() for k, v in cur.items()})


def _three_steps(hip, monkeypatch, shape, hatless):
    from pykg2vec_amd import kernels as K
    tr = _trainer(hip, monkeypatch, shape, hatless, 3)
    assert K.pull_hatless() == (hatless == "1")
    tr.generator.start_one_epoch(3)
    tr.loss_buf.zero_()
    out = {"pair": _shape_one_pair(tr, shape)}
    for k in range(3):   # (the records and codes are those of the last step: looked at after every one)
        tr.step_next_batches(1)
        _state(tr, out, "step%d" % k)
    assert tr.flat.step == 3 and tr._pull.hats_stale == (hatless == "1") and tr._pull.inv_stale == (hatless != "1")
    return out


def _codes_of_pair(codes, d, pair):
    """[lanes, 2, 4] direction codes (residual: positive / negative; element of the lane's float4) of one pair."""
    from pykg2vec_amd import kernels as K
    lanes = K.pull_partial_stride(d) // 4
    c = codes.cpu().numpy().view(np.uint16)[pair * lanes:(pair + 1) * lanes].astype(np.int64)
    return np.stack([[(c >> (8 * res + 2 * e)) & 3 for e in range(4)] for res in (0, 1)], 0).transpose(2, 0, 1)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stored_inverse_norms_change_no_byte(hip, monkeypatch, shape):
    ref = _three_steps(hip, monkeypatch, shape, "0")
    assert float(ref["step2/moment2"].abs().max()) > 0 and float(ref["step2/recs"].abs().max()) > 0   # (the steps did run)
    d, special, q = SHAPES[shape][3], SHAPES[shape][6], ref.pop("pair")
    if special == "signed_zeros":   # the construction holds in the reference arm: pair 0 is active and codes 0 where its residual is +-0
        assert float(ref["step0/recs"][4 * q]) != 0.0
        pos = _codes_of_pair(ref["step0/codes"], d, q)[:, 0, :].reshape(-1)   # element 4 * lane + e
        assert all(pos[e] == 0 for e in ZERO_AT + NEGZERO_AT) and (pos[:d] != 0).sum() >= d - 8
    if special == "subnormals":     # ... and here its subnormal half carries codes of both signs (a sum of three may cancel to 0)
        assert float(ref["step0/recs"][4 * q]) != 0.0
        pos = _codes_of_pair(ref["step0/codes"], d, q)[:d // 8, 0, :]
        assert (pos == 1).sum() >= d // 16 and (pos == 3).sum() >= d // 16
    got = _three_steps(hip, monkeypatch, shape, "1")
    assert got.pop("pair") == q
    for k in ref:
        assert torch.equal(ref[k], got[k]), (shape, k)


def _mixed_run(hip, monkeypatch, hatless):
    """Three two-phase steps, one one-phase step (its owners write norms but no inverse norms), two more two-phase steps, on one state."""
    tr = _trainer(hip, monkeypatch, "odd_pairs_d100", hatless, 6)
    tr.generator.start_one_epoch(6)
    tr.loss_buf.zero_()
    ps = tr._pull_state()[0]
    ps.sync_in()
    tr.step_next_batches(3)
    assert ps.hats_stale == (hatless == "1") and not (hatless == "1" and ps.inv_stale)
    tr.switches["pull_dir"] = False            # KGE_PULL_DIR=0: one one-phase step
    tr.step_next_batches(1)
    assert tr._pull is ps and not ps.plan_two_phase and not ps.hats_stale and ps.inv_stale
    tr.switches["pull_dir"] = True
    tr.step_next_batches(2)
    assert tr._pull is ps and ps.plan_two_phase and tr.flat.step == 6 and ps.inv_stale == (hatless != "1")
    out = {}
    _state(tr, out, "end")
    tr.sync_model()
    _state(tr, out, "synced")
    return out


def test_inverse_norms_stay_valid_across_a_one_phase_step(hip, monkeypatch):
    ref = _mixed_run(hip, monkeypatch, "0")
    assert float(ref["end/recs"].abs().max()) > 0
    got = _mixed_run(hip, monkeypatch, "1")
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
