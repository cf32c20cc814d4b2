"""OctonionE on the HIP path (csrc/kge_octonion.hip): parity with the frozen reference outputs in
tests/golden/ref_octonione{,_neg3}.npz, the fused step at larger shapes against the float64 restatement of
test_octonione_model.py, the fused sampler, hipGraph replay, the rank sweeps and the refusals of the other step kinds."""
import numpy as np
import pytest
import torch

import kge_oracle as ko
from golden_util import Case, close, rank_band_ok, zipf_ids
from test_octonione_model import ENT, REL, energy64, pointwise_loss64

pytestmark = pytest.mark.gpu

NAMES = ["octonione", "octonione_neg3"]
GRAD_TOL = dict(atol=2e-5, rtol=1e-4)
TABLES = ENT + REL


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def case(name):
    c = Case(name)
    c.model, c.pointwise = "octonione", True   # (golden_util.POINTWISE predates this model)
    return c


def named_tables(hip, m):
    return [(k, p) for k, p in hip.table_parameters(m) if not k.startswith("rel_w")]


def batch_tensors(hip, c, s):
    return [hip.dev(x) for x in c.batch(s)]


# ---------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_reference_golden(hip, name):
    c = case(name)
    m = hip.model_from_case(c)
    b = batch_tensors(hip, c, 0)
    with torch.no_grad():
        got = m(b[0], b[1], b[2]).cpu().numpy()
    assert close(got, c.z["scores0"], atol=2e-5, rtol=2e-5), np.abs(got - c.z["scores0"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_autograd_path_matches_reference_grads(hip, name):
    """torch.ops.kge.score's backward hands separate zeros_like gradients: the packed-block route of kernels.octonion_desc."""
    c = case(name)
    m = hip.model_from_case(c)
    b = batch_tensors(hip, c, 0)
    m.train()
    loss = m.loss(m(b[0], b[1], b[2]), b[3].float()) + m.get_reg(b[0], b[1], b[2])
    loss.backward()
    assert close(loss.item(), c.z["loss0"], atol=2e-5, rtol=2e-5), (loss.item(), c.z["loss0"])
    for k, p in named_tables(hip, m):
        ref = c.z["grad0." + k]
        assert np.allclose(p.grad.cpu().numpy(), ref, **GRAD_TOL), (k, np.abs(p.grad.cpu().numpy() - ref).max())
    assert not m.rel_w_embedding.weight.grad.any()


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_matches_reference_loss_and_grads(hip, name):
    from pykg2vec_amd.trainer import Trainer
    c = case(name)
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    m = hip.model_from_case(c)
    tr = Trainer(m, cfg)
    tr.build_model()
    assert tr.step_path() == "generic" and tr._fused_pointwise_ok()
    # zero-copy: the descriptor points into the flat buffers
    assert tr._desc.tables[0] == tr.flat.views[0].data_ptr() and tr._desc.tables[1] == tr.flat.views[8].data_ptr()
    assert tr._desc.grads[0] == tr.flat.grad_views[0].data_ptr() and not tr._desc._after
    loss = tr.train_step_pointwise(*batch_tensors(hip, c, 0))
    assert close(loss.item(), c.z["loss0"], atol=2e-5, rtol=2e-5), (loss.item(), c.z["loss0"])
    for (k, _), g in zip(named_tables(hip, m), tr.flat.grad_views):
        ref = c.z["grad0." + k]
        assert np.allclose(g.cpu().numpy(), ref, **GRAD_TOL), (k, np.abs(g.cpu().numpy() - ref).max())
    assert not tr.flat.grad_views[16].any()


@pytest.mark.parametrize("name,opt", [(n, o) for n in NAMES for o in ("sgd", "adam", "adagrad", "rms")])
def test_three_fused_training_steps_match_reference_weights(hip, name, opt):
    from pykg2vec_amd.trainer import Trainer
    c = case(name)
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.05)
    m = hip.model_from_case(c)
    tr = Trainer(m, cfg)
    tr.build_model()
    losses = []
    for s in range(3):
        losses.append(tr.train_step_pointwise(*batch_tensors(hip, c, s)).item())
        tr._reduce_and_step()
    assert close(np.asarray(losses), c.z["%s.losses" % opt], atol=3e-5, rtol=3e-5), (losses, c.z["%s.losses" % opt])
    tol = 2e-3 if opt == "rms" else 1e-4
    for k, p in hip.table_parameters(m):
        ref = c.z["%s.final.%s" % (opt, k)]
        got = p.detach().cpu().numpy()
        if k.startswith("rel_w"):
            assert np.array_equal(got, c.z["init." + k]) and np.array_equal(ref, c.z["init." + k]), k
            continue
        bad = ~np.isclose(got, ref, atol=tol, rtol=1e-4)
        if opt == "rms":   # the rule of test_hip_parity.py: isolated entries whose gradient is a rounding residue may move
            assert bad.mean() < 2e-3, (k, bad.sum(), np.abs(got - ref).max())
            continue
        assert not bad.any(), (k, bad.sum(), np.abs(got - ref).max())


@pytest.mark.parametrize("name", NAMES)
def test_eval_sweep_scores_and_ranks_match_reference(hip, name):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.evaluator import Evaluator
    c = case(name)
    m = hip.model_from_case(c, "adam.final.")
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    sw = K.eval_sweep_scores(m.make_desc(), hip.dev(c.test[:4])).cpu().numpy()
    assert close(sw, c.z["eval.sweeps"], atol=2e-5, rtol=2e-5), np.abs(sw - c.z["eval.sweeps"]).max()
    ev = Evaluator(m, cfg)
    n = len(c.z["eval.rank_head"])
    ranks = ev.rank_all(c.test, n).cpu().numpy()
    ref = np.stack([c.z["eval.rank_head"], c.z["eval.rank_tail"], c.z["eval.frank_head"], c.z["eval.frank_tail"]])
    scores = K.eval_sweep_scores(m.make_desc(), hip.dev(c.test[:n])).cpu().numpy()
    E = c.E
    with torch.no_grad():   # the sweep's energies are the forward's, to fp32 rounding
        for i, (h, r, t) in enumerate(c.test[:n]):
            ft = m(hip.dev(np.full(E, h)), hip.dev(np.full(E, r)), hip.dev(np.arange(E))).cpu().numpy()
            fh = m(hip.dev(np.arange(E)), hip.dev(np.full(E, r)), hip.dev(np.full(E, t))).cpu().numpy()
            assert np.allclose(scores[2 * i], ft, atol=2e-5, rtol=2e-5) and np.allclose(scores[2 * i + 1], fh, atol=2e-5, rtol=2e-5)
    hr_t, tr_h = c.filters()
    equal = 0
    for i, (h, r, t) in enumerate(c.test[:n]):
        rt = ko.rank_from_scores(scores[2 * i], int(t), hr_t[(int(h), int(r))])
        rh = ko.rank_from_scores(scores[2 * i + 1], int(h), tr_h[(int(t), int(r))])
        assert (ranks[1, i], ranks[3, i]) == rt and (ranks[0, i], ranks[2, i]) == rh   # exact function of our own energies
        for row, true, a, b in ((scores[2 * i], int(t), 1, 3), (scores[2 * i + 1], int(h), 0, 2)):
            for j in (a, b):
                ok, near = rank_band_ok(row, true, ranks[j, i], ref[j, i])
                assert ok, (name, i, j, ranks[:, i], ref[:, i], near)
                equal += int(ranks[j, i] == ref[j, i])
    assert equal >= 4 * n - 2, (equal, 4 * n)
    metrics = ev.test(c.test, n, epoch=0)
    assert np.isclose(metrics["fmr"], c.z["eval.fmr"], rtol=0.02)


@pytest.mark.parametrize("name", NAMES)
def test_one_sided_sweeps_and_rank_hooks(hip, name):
    from pykg2vec_amd import kernels as K
    c = case(name)
    m = hip.model_from_case(c, "adam.final.")
    trips = c.test[:5]
    both = K.eval_sweep_scores(m.make_desc(), hip.dev(trips))
    tail = K.eval_sweep_scores_side(m.make_desc(), hip.dev(trips), 0)
    head = K.eval_sweep_scores_side(m.make_desc(), hip.dev(trips), 1)
    assert torch.equal(tail, both[0::2]) and torch.equal(head, both[1::2])
    h, r, t = (hip.dev(trips[:1, i]) for i in range(3))
    ids = m.predict_tail_rank(h, r, topk=c.E)
    assert torch.equal(both[0][ids[0]], torch.sort(both[0], descending=True).values)
    ids = m.predict_head_rank(t, r, topk=c.E)
    assert torch.equal(both[1][ids[0]], torch.sort(both[1], descending=True).values)


def test_packed_and_block_descriptors_agree(hip):
    """Tables moved out of the block layout go through packed copies; scores and accumulated gradients are the same."""
    from pykg2vec_amd import kernels as K
    c = case("octonione")
    m = hip.model_from_case(c)
    w = [p.weight.detach() for p in m.parameter_list]
    loose = [x.clone() for x in w]
    b = batch_tensors(hip, c, 0)
    ds = torch.linspace(-1, 1, b[0].numel(), device=b[0].device)
    outs = []
    for tabs in (w, loose):
        grads = [torch.full_like(x, 0.25) for x in tabs]   # accumulation: the packed route must carry the old values in and out
        desc = K.octonion_desc(tabs, grads, tot_entity=c.E, tot_relation=c.R, dim=m.hidden_size)
        assert (desc.tables[0] == tabs[0].data_ptr()) == (tabs is w)   # block tables by address, loose ones packed
        s = K.score_forward(desc, b[0], b[1], b[2])
        K.score_backward(desc, b[0], b[1], b[2], ds)
        outs.append((s, grads))
    assert torch.equal(outs[0][0], outs[1][0])
    for ga, gb in zip(outs[0][1], outs[1][1]):
        assert torch.allclose(ga, gb, atol=1e-6, rtol=1e-5)
    assert torch.equal(outs[1][1][16], torch.full_like(w[16], 0.25))


# ---------------------------------------------------------------- larger shapes against float64
SHAPES = [(d, B, neg) for d in (50, 100, 256, 1000) for B in (128, 4096, 50000) for neg in (1, 4)]


def random_model(hip, E, R, d, seed):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    m = hip.model_from_params("octonione", {}, dict(hidden_size=d, lmbda=0.05), E, R)
    with torch.no_grad():   # rows and relation elements of varying size: the normalisation backward is exercised
        for p in m.parameter_list:
            p.weight.mul_(torch.from_numpy(rng.uniform(0.5, 2.0, (p.weight.shape[0], 1)).astype(np.float32)).to(p.weight.device))
    return m


def bundles(rng, E, R, B, neg, rel_ids=None):
    """B positives each followed by neg corruptions of the head or the tail (the generator's pointwise layout)."""
    r = rel_ids if rel_ids is not None else rng.integers(R, size=B)
    pos = np.stack([rng.integers(E, size=B), r, rng.integers(E, size=B)], 1)
    rows = np.repeat(pos, 1 + neg, 0)
    y = np.tile(np.array([1] + [-1] * neg, np.int64), B)
    neg_rows = np.nonzero(y < 0)[0]
    side = rng.random(len(neg_rows)) < 0.5
    rows[neg_rows[side], 0] = rng.integers(E, size=side.sum())
    rows[neg_rows[~side], 2] = rng.integers(E, size=(~side).sum())
    return rows[:, 0], rows[:, 1], rows[:, 2], y


def check_step_vs_float64(hip, m, E, R, batch, B):
    """One fused step (Trainer, zero-copy descriptor) against the float64 restatement, evaluated on the GPU in row chunks (the
    loss is a sum over rows, so chunked autograd accumulates the same gradients)."""
    from pykg2vec_amd.trainer import Trainer
    hp = dict(hidden_size=m.hidden_size, lmbda=m.lmbda, neg_rate=int((batch[3] < 0).sum() // (batch[3] > 0).sum()))
    P = {k.split(".")[0]: p.detach().double().clone().requires_grad_(True) for k, p in named_tables(hip, m)}
    ids = [hip.dev(x) for x in batch]
    n = ids[0].numel()
    loss64 = 0.0
    for a in range(0, n, 16384):
        sl = [x[a:a + 16384] for x in ids]
        part = pointwise_loss64(P, *sl[:3], sl[3].double(), m.lmbda) * (sl[0].numel() / n)   # means over n rows / n*d elements
        part.backward()
        loss64 += part.item()
    trip = np.stack(batch[:3], 1)
    cfg = hip.make_config(E, R, hp, trip, trip[:4], trip[:4], batch_size=B)
    tr = Trainer(m, cfg)
    tr.build_model()
    assert tr.step_path() == "generic"
    with torch.no_grad():
        s32 = m(ids[0][:4096], ids[1][:4096], ids[2][:4096]).double()
        e64 = energy64(P, ids[0][:4096], ids[1][:4096], ids[2][:4096])
        assert torch.allclose(s32, e64, rtol=1e-5, atol=1e-5 * float(e64.abs().max())), (s32 - e64).abs().max()
    loss = tr.train_step_pointwise(*ids)
    assert np.isclose(loss.item(), loss64, rtol=1e-5, atol=1e-6), (loss.item(), loss64)
    for (k, _), g in zip(named_tables(hip, m), tr.flat.grad_views):
        ref = P[k.split(".")[0]].grad
        scale = max(1e-6, float(ref.abs().max()))
        err = float((g.double() - ref).abs().max())
        assert torch.allclose(g.double(), ref, atol=1e-4 * scale, rtol=1e-3), (k, err, scale)


@pytest.mark.parametrize("d,B,neg", SHAPES)
def test_step_vs_float64_restatement(hip, d, B, neg):
    E, R = 3000, 40
    m = random_model(hip, E, R, d, seed=d * 7 + B + neg)
    check_step_vs_float64(hip, m, E, R, bundles(np.random.default_rng(B + d + neg), E, R, B, neg), B)


@pytest.mark.parametrize("d,neg", [(50, 1), (256, 4)])
def test_step_vs_float64_on_zipf_skewed_relations(hip, d, neg):
    """A few hub relations take most bundles: their gradient rows take thousands of atomic row-adds per step."""
    E, R, B = 3000, 40, 4096
    rng = np.random.default_rng(d + neg)
    m = random_model(hip, E, R, d, seed=d + 1)
    rel = zipf_ids(rng, B, R, 1.2)
    check_step_vs_float64(hip, m, E, R, bundles(rng, E, R, B, neg, rel_ids=rel), B)


@pytest.mark.parametrize("neg", [1, 3])
def test_fused_sampler_step_equals_sample_then_step(hip, neg):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    c = case("octonione")
    hp = dict(c.hp, neg_rate=neg)
    cfg = hip.make_config(c.E, c.R, hp, c.train, c.valid, c.test, batch_size=64)
    res = []
    for fused in (False, True):
        m = hip.model_from_case(c)
        tr = Trainer(m, cfg)
        tr.build_model()
        assert tr._fused_pointwise_ok() and tr.step_path() == "generic"
        gen = tr._new_generator()
        tr.generator = gen
        tr.loss_buf.zero_()
        lm, rt = m.kernel_lmbda(), m.kernel_reg_type()
        if fused:
            K.train_pointwise_logistic_sampled(tr._desc, gen.triples, gen.perm, 128, 64, neg, None, gen.slots, 11, 999, lm, rt, tr.loss_buf)
        else:
            b = K.sample_batch(gen.triples, gen.perm, 128, 64, neg, c.E, None, gen.slots, 11, 999, pointwise=True)
            K.train_pointwise_logistic(tr._desc, *b[:4], lm, rt, tr.loss_buf, bundle=1 + neg)
        res.append((K.read_loss(tr.loss_buf).item(), [g.cpu().numpy().copy() for g in tr.flat.grad_views]))
    assert np.isclose(res[0][0], res[1][0], rtol=1e-5)
    for a, b in zip(res[0][1], res[1][1]):
        assert np.allclose(a, b, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_graph_replayed_epochs_equal_eager_epochs(hip, opt):
    from pykg2vec_amd.trainer import Trainer
    c = case("octonione")
    out = []
    for use_graph in (False, True):
        cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.02, batch_size=16)
        m = hip.model_from_case(c)
        tr = Trainer(m, cfg, use_graph=use_graph)
        tr.build_model()
        tr.generator = tr._new_generator()
        losses = [tr.train_model_epoch(e) for e in range(3)]
        assert (tr._graph is not None) == use_graph and tr.step_path() == "generic"
        out.append((losses, {k: p.detach().cpu().numpy() for k, p in hip.table_parameters(m)}))
    (l0, p0), (l1, p1) = out
    assert np.allclose(l0, l1, rtol=2e-4), (l0, l1)
    for k in p0:   # rows sum under float atomics: summation order only
        assert np.allclose(p0[k], p1[k], atol=2e-4, rtol=1e-3), (k, np.abs(p0[k] - p1[k]).max())


def test_other_step_kinds_and_wide_rows_are_refused(hip):
    from pykg2vec_amd import _lib as L
    from pykg2vec_amd import kernels as K
    c = case("octonione")
    m = hip.model_from_case(c)
    grads = [torch.zeros_like(p.weight) for p in m.parameter_list]
    desc = m.make_desc(None, grads)
    b = batch_tensors(hip, c, 0)
    with pytest.raises(L.KgeHipError, match="pointwise logistic step only"):
        K.train_pairwise_hinge(desc, b[0], b[1], b[2], b[0], b[1], b[2], 1.0, K.new_loss_buffer(b[0].device))
    assert K.own_groups_per_block("octonione", 12) == 0
    wide = hip.model_from_params("octonione", {}, dict(hidden_size=2049, lmbda=0.1), 4, 2)
    with pytest.raises(L.KgeHipError, match="hidden sizes"):
        K.score_forward(wide.make_desc(), hip.dev([0]), hip.dev([1]), hip.dev([2]))
    with pytest.raises(L.KgeHipError, match="neg_rate"):   # 1 + neg_rate rows must fit the 32-lane group at d <= 256
        tr_trip = hip.dev(c.train)
        K.train_pointwise_logistic_sampled(desc, tr_trip, hip.dev(np.arange(len(c.train))), 0, 4, 32, None, None, 1, 0,
                                           m.kernel_lmbda(), m.kernel_reg_type(), K.new_loss_buffer(b[0].device))
