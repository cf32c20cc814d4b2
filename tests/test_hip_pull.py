"""The owner-computes ("pull") training step (csrc/kge_pull.hip): no atomics, optimiser fused, bit-reproducible.
Held to (a) the live reference's golden post-optimiser weights on its golden batches, (b) the push path (atomic
scatter + dense optimiser sweep) on the batch the fused sampler draws at BASELINE size, (c) itself, bit for bit,
across runs."""
import numpy as np
import pytest
import torch

import kge_oracle as ko
from golden_util import Case, close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


PULL_WEIGHT_ATOL = 8e-6   # 2x the largest deviation recorded over the 80 cases (3.6e-6, RMSprop / L2; profiles/r04_weight_agreement.json)


@pytest.mark.parametrize("segment,compact", [(None, False), (2, False), (1, False), (None, True), (1, True)])
@pytest.mark.parametrize("opt", ["sgd", "adam", "adagrad", "rms"])
@pytest.mark.parametrize("name", ["transe_l1", "transe_l2", "transm_l1", "transm_l2"])
def test_three_pull_steps_match_reference_weights(hip, name, opt, segment, compact):
    """Golden batches of the live reference, three steps: losses and post-optimiser tables (tests/golden/ref_transe_*).
    segment=2 cuts almost every row's incidence list into several work items that combine through LDS inside one
    workgroup; segment=1 additionally pushes the relation rows (> 8 incidences) through global partial sums + the
    finishing kernel."""
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    c = Case(name)
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.05)
    m = hip.model_from_case(c)
    tr = Trainer(m, cfg)
    tr.build_model()
    losses = []
    for s in range(3):
        b = [hip.dev(x) for x in c.batch(s)]
        tr.loss_buf.zero_()
        tr.pull_step_explicit(*b, segment=segment, compact=compact)   # compact: only touched rows listed, the rest implicit
        losses.append(K.read_loss(tr.loss_buf).item())
    assert close(np.asarray(losses), c.z["%s.losses" % opt], atol=3e-5, rtol=3e-5), (losses, c.z["%s.losses" % opt])
    for k, p in hip.table_parameters(m):
        ref = c.z["%s.final.%s" % (opt, k)]
        got = p.detach().cpu().numpy()
        # no atomics, fixed summation order: held to ~2x the largest deviation from the live reference's weights ever observed
        # (profiles/r04_weight_agreement.json; the push path's atomics needed 1e-4)
        hip.record_max("weight_agreement", "pull_3_steps/%s/%s" % (name, opt), np.abs(got - ref).max())
        assert np.allclose(got, ref, atol=PULL_WEIGHT_ATOL, rtol=0), (k, np.abs(got - ref).max())


@pytest.mark.parametrize("segment,compact", [(None, False), (2, False), (1, False), (1, True)])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("name", ["transe_l1", "transe_l2", "transm_l1", "transm_l2"])
def test_two_phase_step_is_the_one_phase_step_bit_for_bit(hip, monkeypatch, name, opt, segment, compact):
    """KGE_PULL_DIR=1: k_pull_eval evaluates every pair once and the owners sum the pairs' records (2-bit direction codes) instead of
    re-evaluating them.  Same coefficients, same fused multiply-adds in the same order: the tables, optimiser state and the golden
    weights of the live reference must come out identical to the one-phase step.  The form exists for L1 only (both evaluate-once
    forms of L2 measured slower and were removed, round 5): an L2 model ignores the switch and both arms run the one-phase step."""
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    c = Case(name)
    out = []
    for two_phase in ("0", "1"):
        monkeypatch.setenv("KGE_PULL_DIR", two_phase)
        cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.05)
        m = hip.model_from_case(c)
        tr = Trainer(m, cfg)
        tr.build_model()
        assert tr._pull_two_phase() == (two_phase == "1" and name.endswith("_l1"))
        losses = []
        for s in range(3):
            b = [hip.dev(x) for x in c.batch(s)]
            tr.loss_buf.zero_()
            tr.pull_step_explicit(*b, segment=segment, compact=compact)
            losses.append(K.read_loss(tr.loss_buf).item())
        assert close(np.asarray(losses), c.z["%s.losses" % opt], atol=3e-5, rtol=3e-5), (two_phase, losses)
        out.append((tr.flat.param.clone(), None if tr.flat.state1 is None else tr.flat.state1.clone()))
    assert torch.equal(out[0][0], out[1][0])
    if out[0][1] is not None:
        assert torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("l1,opt", [(True, "adam"), (False, "adam"), (True, "sgd")])
def test_two_phase_epochs_equal_one_phase_epochs_at_baseline_size(hip, world, l1, opt, monkeypatch):
    """Two epochs of four B = 32 768 steps through kge_pull_run (ride-along sampler without visit descriptors, bucket overflow
    ranking, multi-item relation rows): byte-identical tables and optimiser state, equal losses."""
    res = []
    for two_phase in ("0", "1"):
        monkeypatch.setenv("KGE_PULL_DIR", two_phase)
        tr, m, cfg = _trainer(hip, world, l1, opt, True, monkeypatch)
        losses = [tr.train_model_epoch(e) for e in range(2)]
        assert (tr._pull.direction is not None) == (two_phase == "1" and l1)
        res.append((losses, tr.flat.param.clone(), None if tr.flat.state1 is None else tr.flat.state1.clone()))
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5), (res[0][0], res[1][0])
    # the two-phase run cuts the incidence lists into items of 32 instead of 8: the partial sums of long rows group differently.
    # L1 gradients are sums of +-1 / +-0.5 (exact in fp32 in any order): byte-identical.  L2: rounding-level differences.
    # (Adam turns a rounding-residue gradient into a +-lr step: isolated entries may differ, as in the pull-vs-push test above)
    same = torch.equal if l1 else (lambda a, b: float((~torch.isclose(a, b, atol=2e-5, rtol=1e-4)).float().mean()) <= 2e-3)
    assert same(res[0][1], res[1][1])
    if res[0][2] is not None:
        assert same(res[0][2], res[1][2])


E, R, D, B = 14951, 1345, 100, 32768


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(1234)
    n_train = 4 * B + 100
    train = np.stack([rng.integers(E, size=n_train), rng.integers(R, size=n_train), rng.integers(E, size=n_train)], 1)
    test = np.stack([rng.integers(E, size=64), rng.integers(R, size=64), rng.integers(E, size=64)], 1)
    P = ko.init_params("transe", rng, tot_entity=E, tot_relation=R, hidden_size=D)
    return train, test, P


def _trainer(hip, world, l1=True, opt="adam", pull=True, monkeypatch=None):
    from pykg2vec_amd.trainer import Trainer
    train, test, P = world
    hp = dict(hidden_size=D, l1_flag=l1, margin=1.0)
    cfg = hip.make_config(E, R, hp, train[:1], test[:16], test, optimizer=opt, lr=0.01, batch_size=B)
    cfg.knowledge_graph.cache["triplets_train"] = train
    cfg.tot_train_triples = len(train)
    m = hip.model_from_params("transe", P, hp, E, R)
    monkeypatch.setenv("KGE_PULL", "1" if pull else "0")
    tr = Trainer(m, cfg, use_graph=False)
    tr.build_model()
    tr.generator = tr._new_generator()
    return tr, m, cfg


@pytest.mark.parametrize("l1,opt", [(True, "adam"), (False, "sgd"), (True, "adagrad")])
def test_pull_epoch_equals_push_epoch_at_baseline_size(hip, world, l1, opt, monkeypatch):
    """Same generator seed => same batches and the same Philox draws on both paths: after an epoch of 4 steps at
    B = 32768 the tables must agree to fp32 summation-order noise, and the epoch losses too."""
    out = []
    for pull in (False, True):
        tr, m, cfg = _trainer(hip, world, l1, opt, pull, monkeypatch)
        assert tr._pull_ok() == pull
        loss = tr.train_model_epoch(0)
        out.append((loss, [p.detach().clone() for _, p in hip.table_parameters(m)]))
    assert np.isclose(out[0][0], out[1][0], rtol=2e-5), (out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        if opt == "adam":
            # Adam moves a weight by ~lr * sign(g) however small g is: entries whose gradient is a rounding residue of
            # cancelling contributions (summation order differs between atomics and the fixed pull order) may land
            # elsewhere -- they are isolated; everything else must agree
            bad = (a - b).abs() > 2e-5 + 1e-4 * b.abs()
            assert bad.float().mean().item() < 1e-2, (bad.sum().item(), (a - b).abs().max().item())
        else:
            assert torch.allclose(a, b, atol=2e-5, rtol=1e-4), (a - b).abs().max().item()


def test_pull_step_matches_oracle_on_its_sampled_batch(hip, world, monkeypatch):
    """One pull step at full size against the numpy oracle's gradients + Adam on the batch the sampler drew."""
    from pykg2vec_amd import kernels as K
    tr, m, cfg = _trainer(hip, world, True, "adam", True, monkeypatch)
    train, test, P = world
    gen = tr.generator
    cfg.tot_train_triples = B   # one step
    loss = tr.train_model_epoch(0)
    batch = K.sample_batch(gen.triples, gen.perm, 0, B, 1, E, None, gen.slots, gen.seed, 0)
    nb = tuple(a.cpu().numpy() for a in batch)
    loss_ref, G_ref, _, _ = ko.train_step_grads("transe", P, nb, l1_flag=True, margin=1.0)
    assert np.isclose(loss, loss_ref, rtol=2e-5), (loss, loss_ref)
    Pn = {k: v.copy() for k, v in P.items()}
    st = ko.optimizer_init("adam", Pn)
    ko.optimizer_step("adam", Pn, G_ref, st, 0.01)
    for k, p in hip.table_parameters(m):
        got, ref = p.detach().cpu().numpy(), Pn[k.split(".")[0]]
        # Adam's first step moves every touched weight by ~lr * sign(g): only entries whose gradient is a rounding
        # residue of cancelling contributions may land elsewhere -- they are isolated
        bad = np.abs(got - ref) > 1e-5 + 1e-4 * np.abs(ref)
        assert bad.mean() < 2e-3, (k, bad.sum(), np.abs(got - ref).max())


def test_training_is_bit_reproducible(hip, world, monkeypatch):
    """SURVEY.md section 5 (race detection): no atomics on parameters or gradients, fixed summation orders -- two runs
    from the same state produce byte-identical tables, optimiser state and row norms."""
    res = []
    for _ in range(2):
        tr, m, cfg = _trainer(hip, world, True, "adam", True, monkeypatch)
        for e in range(2):
            tr.train_model_epoch(e)
        res.append((tr.flat.param.clone(), tr.flat.state1.clone(), tr.flat.state2.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_pull_untouched_rows_follow_dense_optimizer_semantics(hip, monkeypatch):
    """nn.Embedding is dense (models/Domain.py:8-13): Adam moves rows with momentum even when the batch does not touch
    them; a row nobody touches in step 1 must still equal torch's dense update (zero gradient: unchanged for a fresh
    state) and in step 2 keep decaying its moments."""
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    c = Case("transe_l1")
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer="adam", lr=0.05)
    m = hip.model_from_case(c)
    tr = Trainer(m, cfg)
    tr.build_model()
    b0 = [hip.dev(x) for x in c.batch(0)]
    # second batch: one pair only -> almost every row is untouched but carries momentum from the first step
    b1 = [x[:1].contiguous() for x in [hip.dev(y) for y in c.batch(1)]]
    tr.pull_step_explicit(*b0)
    before = m.ent_embeddings.weight.detach().clone()
    m1 = tr.flat.state1.clone()
    tr.pull_step_explicit(*b1)
    after = m.ent_embeddings.weight.detach()
    touched = set(int(x) for t in (b1[0], b1[2], b1[3], b1[5]) for x in t.cpu().numpy())
    moved = (after != before).any(1).cpu().numpy()
    had_momentum = (m1[:c.E * c.hp["hidden_size"]].view(c.E, -1) != 0).any(1).cpu().numpy()
    for e in range(c.E):
        if e not in touched:
            assert moved[e] == had_momentum[e], e


@pytest.mark.parametrize("l1", [True, False])
def test_gradient_mode_equals_the_atomic_gradient(hip, world, l1, monkeypatch):
    """kge_pull_step in KGE_OPT_GRADIENT mode (what data-parallel ranks run) writes, for every row, the dense gradient the
    atomic-scatter kernel accumulates for the same sampled batch."""
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import PullState
    tr, m, cfg = _trainer(hip, world, l1=l1, opt="sgd", pull=False, monkeypatch=monkeypatch)
    gen = tr.generator
    gen.start_one_epoch(1)
    tr.flat.grad.zero_()
    tr._accumulate_next_batch()                      # push kernel: batch 0, Philox offset 0
    want = tr.flat.grad.clone()
    loss_push = K.read_loss(tr.loss_buf).item()
    idx = gen.pull_index()
    ps = PullState(tr.flat, m, idx.batch_size, idx.max_slots, grad_only=True)
    ps.refresh_norms()
    pairs, inc, items, multi = idx.batch(0)
    K.pull_sample(pairs, idx.inv(0), E, gen.bern, gen.slots, gen.seed, 0, ps.lists[0])
    tr.flat.grad.fill_(7.0)                          # every row must be overwritten
    tr.loss_buf.zero_()
    K.pull_step(tr._desc, ps.tables[1], ps.hats[0], None, ps.norms[0], None, None, None, pairs, ps.lists[0], items, inc,
                ps.partials, multi, cfg.margin, "gradient", 0.0, 1, tr.loss_buf, dense_skip=idx.skip(0))
    got = tr.flat.grad
    assert np.isclose(K.read_loss(tr.loss_buf).item(), loss_push, rtol=2e-5)
    n = E * D + R * D
    assert torch.allclose(got[:n], want[:n], atol=2e-5, rtol=1e-4), (got[:n] - want[:n]).abs().max().item()


@pytest.mark.parametrize("E,R,B,nb,seg,gpb,compact,slice_", [
    (53, 7, 32, 3, 8, 8, False, None), (53, 7, 64, 2, 2, 8, None, None), (40, 3, 200, 2, 1, 8, False, None),
    (300, 5, 1000, 2, 8, 4, False, None), (14951, 1345, 4096, 3, 8, 8, None, None), (14951, 1345, 32768, 2, 8, 8, None, None),
    (14951, 1345, 128, 20, 8, 8, None, None),       # compact: only touched rows listed + bitmap
    (40943, 11, 5000, 3, 8, 4, None, None),         # C2 shape: relation lists of ~450 incidences -> global partial slots
    (500, 20, 256, 4, 8, 8, None, (128, 128)),      # a data-parallel rank's slice of every batch
    (17, 2, 4096, 2, 8, 8, False, None),            # tiny entity set: every row is long
    (2000, 1, 2048, 1, 16, 16, False, None)])       # one relation, 16-lane owner groups
def test_device_built_index_equals_the_numpy_one(hip, E, R, B, nb, seg, gpb, compact, slice_):
    """csrc/kge_index.hip (kge_pull_index_build: keys -> batched bitonic sorts -> row list -> placement) against
    generator.build_pull_batch, the numpy statement of the same layout rule: identical arrays for every batch."""
    rng = np.random.default_rng(E * 31 + B)
    n_train = nb * B + 17
    train = np.stack([rng.integers(E, size=n_train), rng.integers(R, size=n_train), rng.integers(E, size=n_train)], 1)
    perm = rng.permutation(n_train)
    _device_index_equals_host_index(hip, train, perm, E, R, B, nb, seg, gpb, compact, slice_)


@pytest.mark.parametrize("E,R,B,nb,seg,gpb,compact,draw", [
    (14951, 1345, 32768, 2, 8, 8, None, "zipf"),    # C1 sizes, Zipf(0.9) entities / Zipf(1.0) relations: hubs of thousands
    (14951, 1345, 32768, 2, 8, 8, True, "zipf"),
    (14951, 1345, 4096, 2, 1, 8, None, "hub"),      # one entity holds over half of every batch's incidences
    (14951, 1345, 4096, 2, 8, 8, None, "hub"),
    (14951, 1345, 4096, 2, 8, 8, True, "hub"),
    (14951, 1345, 4096, 2, 1, 8, True, "hub")])
def test_device_built_index_equals_the_numpy_one_on_skewed_ids(hip, E, R, B, nb, seg, gpb, compact, draw):
    """The same comparison on heavy-tailed batches: hub rows are cut into hundreds to thousands of items and listed in `multi`."""
    from golden_util import skewed_triples
    rng = np.random.default_rng(E * 37 + B + seg)
    n_train = nb * B + 17
    if draw == "zipf":
        train = skewed_triples(rng, n_train, E, R)
    else:
        train = np.stack([rng.integers(E, size=n_train), rng.integers(R, size=n_train), rng.integers(E, size=n_train)], 1)
        train[:, 0] = 4321
        train[rng.random(n_train) < 0.55, 2] = 4321
    perm = rng.permutation(n_train)
    multi = _device_index_equals_host_index(hip, train, perm, E, R, B, nb, seg, gpb, compact, None)
    assert multi > 0


def _device_index_equals_host_index(hip, train, perm, E, R, B, nb, seg, gpb, compact, slice_):
    """Both builders on batches b = train[perm[b * B + lo : b * B + lo + n]]: identical arrays; returns the rows listed in `multi`."""
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.generator import PullIndex
    lo, n = slice_ if slice_ is not None else (0, B)
    host = PullIndex([train[perm[b * B + lo:b * B + lo + n]] for b in range(nb)], E, R, "cpu", segment=seg, groups_per_block=gpb,
                     compact=compact)
    devx = PullIndex.build_on_device(K, hip.dev(train), hip.dev(perm), nb, B, lo, n, E, R, segment=seg, groups_per_block=gpb,
                                     compact=compact)
    assert devx.compact == host.compact and devx.max_slots == host.max_slots and devx.n_batches == nb and devx.batch_size == n
    n_multi = 0
    for b in range(nb):
        for name, a, d in zip(("pairs", "inc", "items", "multi"), host.batch(b), devx.batch(b)):
            a, d = a.numpy(), d.cpu().numpy()
            assert a.shape == d.shape, (b, name, a.shape, d.shape)
            assert np.array_equal(a, d), (b, name, np.flatnonzero((a != d).reshape(len(a), -1).any(1))[:8])
        n_multi += len(host.batch(b)[3])
        assert np.array_equal(host.inv(b).numpy(), devx.inv(b).cpu().numpy())
        if host.compact:
            assert np.array_equal(host.skip(b).numpy(), devx.skip(b).cpu().numpy())
    return n_multi
