"""The owner-computes runs (Trainer paths `pull`, `own`, `transx`) through their shared epoch cursor (state.OwnerRunState) and
native loop (run_steps in csrc/kge_api.hip), one case per branch of the three kge_*_run bodies: (a) an epoch enqueued in chunks is
the epoch enqueued by one call, bit for bit; (b) an abandoned epoch followed by a full one equals the same schedule on the
atomic-scatter (push) path, within the limits the path's own whole-epoch test uses."""
import numpy as np
import pytest
import torch

import kge_oracle as ko

pytestmark = pytest.mark.gpu

E, R, D, B, N_BATCHES = 300, 11, 64, 128, 5

# (id, model, path, its switch, further environment, hyper-parameters)
PAIRWISE = dict(hidden_size=D, l1_flag=True, margin=1.0, neg_rate=1)
POINTWISE = dict(hidden_size=D, lmbda=1e-3, neg_rate=1)
CASES = [("transe_one_phase", "transe", "pull", "KGE_PULL", {"KGE_PULL_DIR": "0"}, PAIRWISE),
         ("transe_two_phase", "transe", "pull", "KGE_PULL", {"KGE_PULL_DIR": "1"}, PAIRWISE),
         ("distmult_staged", "distmult", "own", "KGE_PW_PULL", {}, POINTWISE),
         ("distmult_unstaged", "distmult", "own", "KGE_PW_PULL", {"KGE_OWN_STAGED": "0"}, POINTWISE),
         ("cp_generic", "cp", "own", "KGE_PW_PULL", {}, POINTWISE),
         ("transh", "transh", "transx", "KGE_TRANSX_OWN", {}, PAIRWISE)]
# Adam, path against push: (rtol of the epoch loss, allowed fraction of table entries outside the element-wise bound, that bound
# as (atol, rtol)) -- test_pull_epoch_equals_push_epoch_at_baseline_size (strict <), test_own_epochs_equal_push_epochs and
# test_transx_epochs_equal_push_epochs (<=) respectively
PUSH_LIMITS = {"pull": (2e-5, 1e-2, (2e-5, 1e-4)), "own": (3e-5, 2e-3, (2e-5, 1e-4)), "transx": (3e-5, 5e-3, (2e-5, 1e-4))}


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


@pytest.fixture(scope="module")
def worlds():
    out = {}
    for model in ("transe", "distmult", "cp", "transh"):
        rng = np.random.default_rng(11)
        n_train = N_BATCHES * B + 5
        train = np.stack([rng.integers(E, size=n_train), rng.integers(R, size=n_train), rng.integers(E, size=n_train)], 1)
        out[model] = (train, ko.init_params(model, rng, tot_entity=E, tot_relation=R, hidden_size=D))
    return out


def _trainer(hip, worlds, monkeypatch, case, on=True):
    from pykg2vec_amd.trainer import Trainer
    _, model, path, switch, env, hp = case
    train, P = worlds[model]
    for var in ("KGE_STAGED", "KGE_OWN_STAGED", "KGE_PULL_DIR"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    monkeypatch.setenv(switch, "1" if on else "0")
    cfg = hip.make_config(E, R, hp, train, train[:8], train[:8], optimizer="adam", lr=0.01, batch_size=B)
    cfg.tot_train_triples = N_BATCHES * B
    m = hip.model_from_params(model, P, hp, E, R, train=train)
    tr = Trainer(m, cfg, use_graph=False)
    tr.build_model()
    tr.generator = tr._new_generator()
    assert tr.step_path(N_BATCHES) == (path if on else "generic")
    return tr, m


def _tables(hip, m):
    return [p.detach().clone() for _, p in hip.table_parameters(m)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chunked_epochs_are_whole_epochs_bit_for_bit(hip, worlds, monkeypatch, case):
    """Two epochs as one native call each (train_model_epoch) against the same epochs as calls of (1, 2, 2) and (2, 3) steps between
    the same per-epoch prologue and epilogue train_model_epoch runs (loss accumulators zeroed, the pull path's tables re-adopted,
    tables handed back): the same launches with the same arguments, so every table and the loss accumulators are identical."""
    path = case[2]
    tr1, m1 = _trainer(hip, worlds, monkeypatch, case)
    loss1 = []
    for e in range(2):
        tr1.train_model_epoch(e)
        loss1.append(tr1.loss_buf.clone())
    tr2, m2 = _trainer(hip, worlds, monkeypatch, case)
    loss2 = []
    for chunks in ((1, 2, 2), (2, 3)):
        tr2.generator.start_one_epoch(N_BATCHES)
        tr2.loss_buf.zero_()
        if path == "pull":
            tr2._pull_state()[0].sync_in()
        for n in chunks:
            assert tr2.step_path(n) == path
            tr2.step_next_batches(n)
        tr2.sync_model()
        loss2.append(tr2.loss_buf.clone())
    assert tr1.flat.step == tr2.flat.step == 2 * N_BATCHES
    for a, b in zip(_tables(hip, m1), _tables(hip, m2)):
        assert torch.equal(a, b)
    for a, b in zip(loss1, loss2):
        assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_abandoned_epoch_then_full_epoch_equals_push(hip, worlds, monkeypatch, case):
    """Three of five steps, generator.stop(), then a whole epoch: the list set sampled for batch 3 is discarded and the new epoch's
    batch 0 sampled stand-alone.  Against the same schedule on the push path (the path's switch at 0)."""
    from pykg2vec_amd import kernels as K
    path = case[2]
    res = []
    for on in (False, True):
        tr, m = _trainer(hip, worlds, monkeypatch, case, on)
        tr.generator.start_one_epoch(N_BATCHES)
        tr.loss_buf.zero_()
        tr.step_next_batches(3)
        tr.sync_model()
        part = K.read_loss(tr.loss_buf).item()
        tr.generator.stop()
        res.append(([part, tr.train_model_epoch(1)], _tables(hip, m)))
        if on:
            st = {"pull": "_pull", "own": "_own", "transx": "_transx"}[path]
            assert getattr(tr, st).ready == (0, (3 + N_BATCHES) * B)
    loss_rtol, lim, (atol, rtol) = PUSH_LIMITS[path]
    assert np.allclose(res[1][0], res[0][0], rtol=loss_rtol), (res[1][0], res[0][0])
    for a, b in zip(res[1][1], res[0][1]):
        bad = (a - b).abs() > atol + rtol * (a if path == "pull" else b).abs()   # (the pull test scales by the pull tables)
        frac = bad.float().mean().item()
        assert (frac < lim) if path == "pull" else (frac <= lim), (frac, (a - b).abs().max().item())
