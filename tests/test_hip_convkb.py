"""ConvKB on the HIP path (csrc/kge_convkb.hip): parity with the frozen reference outputs in tests/golden/ref_convkb{,_neg3}.npz,
the collapse, the fused step and the rank pass at production size against the float64 restatement of tools/convkb_reference.py, the
ordered fc1 gradients, the fused sampler, hipGraph replay and the public Trainer / Evaluator classes."""
import numpy as np
import pytest
import torch

import kge_oracle as ko
from golden_util import close, rank_band_ok, skewed_triples
from test_convkb_model import GRAD_TOL, NAMES, SCORE_TOL, TRAINED, ConvCase, cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def batch_tensors(hip, c, s):
    return [hip.dev(x) for x in c.batch(s)]


def trainer_for(hip, c, m, **kw):
    from pykg2vec_amd.trainer import Trainer
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, **kw)
    tr = Trainer(m, cfg)
    tr.build_model()
    return tr, cfg


# ---------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_reference_golden(hip, name):
    c = ConvCase(name)
    m = c.build(device="cuda")
    b = batch_tensors(hip, c, 0)
    with torch.no_grad():
        got = m(b[0], b[1], b[2]).cpu().numpy()
    print("max |scores - scores0| =", np.abs(got - c.z["scores0"]).max())
    assert close(got, c.z["scores0"], **SCORE_TOL), np.abs(got - c.z["scores0"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_autograd_path_matches_reference_grads(hip, name):
    c = ConvCase(name)
    m = c.build(device="cuda")
    b = batch_tensors(hip, c, 0)
    m.train()
    loss = m.loss(m(b[0], b[1], b[2]), b[3].float()) + m.get_reg(b[0], b[1], b[2])
    loss.backward()
    assert close(loss.item(), c.z["loss0"], **SCORE_TOL), (loss.item(), c.z["loss0"])
    for k, p in m.named_parameters():
        ref = c.z["grad0." + k]
        assert np.allclose(p.grad.cpu().numpy(), ref, **GRAD_TOL), (k, np.abs(p.grad.cpu().numpy() - ref).max())
    assert all(conv.weight.grad is None and conv.bias.grad is None for conv in m.conv_list)   # fixed inputs


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_matches_reference_loss_and_grads(hip, name):
    c = ConvCase(name)
    m = c.build(device="cuda")
    tr, _ = trainer_for(hip, c, m)
    assert tr.step_path() == "generic" and tr._fused_pointwise_ok()
    assert [tuple(v.shape) for v in tr.flat.views] == [tuple(c.z["init." + k].shape) for k in TRAINED]      # four segments
    assert tr._desc.ent == tr.flat.views[0].data_ptr() and tr._desc.g_fc_b == tr.flat.grad_views[3].data_ptr()   # zero-copy
    loss = tr.train_step_pointwise(*batch_tensors(hip, c, 0))
    assert close(loss.item(), c.z["loss0"], **SCORE_TOL), (loss.item(), c.z["loss0"])
    for k, g in zip(TRAINED, tr.flat.grad_views):
        ref = c.z["grad0." + k]
        assert np.allclose(g.cpu().numpy(), ref, **GRAD_TOL), (k, np.abs(g.cpu().numpy() - ref).max())


@pytest.mark.parametrize("name,opt", [(n, o) for n in NAMES for o in ("sgd", "adam", "adagrad", "rms")])
def test_three_fused_training_steps_match_reference_weights(hip, name, opt):
    c = ConvCase(name)
    m = c.build(device="cuda")
    tr, _ = trainer_for(hip, c, m, optimizer=opt, lr=0.05)
    losses = []
    for s in range(3):
        losses.append(tr.train_step_pointwise(*batch_tensors(hip, c, s)).item())
        tr._reduce_and_step()
    assert close(np.asarray(losses), c.z["%s.losses" % opt], atol=3e-5, rtol=3e-5), (losses, c.z["%s.losses" % opt])
    tol = 2e-3 if opt == "rms" else 1e-4
    sd = m.state_dict()
    for k in TRAINED:                         # fc1 included: the reference's optimiser steps all four
        ref = c.z["%s.final.%s" % (opt, k)]
        got = sd[k].detach().cpu().numpy()
        assert not np.array_equal(ref, c.z["init." + k]), k
        bad = ~np.isclose(got, ref, atol=tol, rtol=1e-4)
        if opt == "rms":   # the rule of test_hip_parity.py: isolated entries whose gradient is a rounding residue may move
            assert bad.mean() < 2e-3, (k, bad.sum(), np.abs(got - ref).max())
            continue
        assert not bad.any(), (k, bad.sum(), np.abs(got - ref).max())


@pytest.mark.parametrize("name", NAMES)
def test_eval_sweeps_ranks_and_metrics_match_reference(hip, name):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.evaluator import Evaluator
    c = ConvCase(name)
    m = c.build("adam.final.", device="cuda")
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    sw = K.eval_sweep_scores(m.make_desc(), hip.dev(c.test[:4])).cpu().numpy()
    print("max |sweeps - eval.sweeps| =", np.abs(sw - c.z["eval.sweeps"]).max())
    assert close(sw, c.z["eval.sweeps"], **SCORE_TOL), np.abs(sw - c.z["eval.sweeps"]).max()
    ev = Evaluator(m, cfg)
    n = len(c.z["eval.rank_head"])
    ranks = ev.rank_all(c.test, n).cpu().numpy()
    ref = np.stack([c.z["eval.rank_head"], c.z["eval.rank_tail"], c.z["eval.frank_head"], c.z["eval.frank_tail"]])
    print("ranks\n", ranks, "\nreference\n", ref)
    assert ranks.shape == (4, 12) and np.array_equal(ranks, ref)          # all 24 ranks and 24 filtered ranks, no exclusions
    metrics = ev.test(c.test, n, epoch=0)
    for key in ("mr", "fmr", "mrr", "fmrr"):
        assert np.isclose(metrics[key], c.z["eval." + key], rtol=1e-5), (key, metrics[key], c.z["eval." + key])
    # the rank hooks of the reference's Evaluator are served by the sweep entry point
    h, r, t = (hip.dev(c.test[:1, i]) for i in range(3))
    tail = K.eval_sweep_scores_side(m.make_desc(), hip.dev(c.test[:1]), 0)[0]
    head = K.eval_sweep_scores_side(m.make_desc(), hip.dev(c.test[:1]), 1)[0]
    assert torch.equal(tail[m.predict_tail_rank(h, r, topk=c.E)[0]], torch.sort(tail, descending=True).values)
    assert torch.equal(head[m.predict_head_rank(t, r, topk=c.E)[0]], torch.sort(head, descending=True).values)


# ---------------------------------------------------------------- production sizes against float64
def random_model(E, R, k, F, widths, seed):
    import pykg2vec_amd as pa
    torch.manual_seed(seed)
    return pa.import_model("convkb")(tot_entity=E, tot_relation=R, hidden_size=k, num_filters=F, filter_sizes=widths, device="cuda").to("cuda")


def params64(m):
    cpu = lambda x: x.detach().cpu().numpy()
    return cr.make_params(cpu(m.ent_embeddings.weight), cpu(m.rel_embeddings.weight), cpu(m.fc1.weight), cpu(m.fc1.bias),
                          [cpu(x.weight) for x in m.conv_list], [cpu(x.bias) for x in m.conv_list])


@pytest.mark.parametrize("widths", [[1, 2], [1, 2, 3], [3, 1, 2]])
def test_collapse_vs_float64(hip, widths):
    from pykg2vec_amd import kernels as K
    m = random_model(50, 7, 100, 50, widths, seed=sum(widths) * 10 + widths[0])
    got = K.convkb_collapse(m.make_desc()).double().cpu().numpy()
    A, c0 = cr.collapse64(params64(m))
    want = np.concatenate([A.reshape(-1), [c0]])
    err = np.abs(got - want).max()
    print("collapse", widths, "max abs err", err, "scale", np.abs(want).max())
    # 150..300 fp32 products of magnitude <= max|A| / terms each, accumulated in fp32: 2^-23 * terms * scale bounds the error
    assert err <= 300 * 2.0 ** -23 * np.abs(want).max(), (err, np.abs(want).max())
    assert torch.equal(K.convkb_collapse(m.make_desc()), K.convkb_collapse(m.make_desc()))     # deterministic


def test_collapse_depends_on_the_order_of_the_widths(hip):
    """The same filters and the same fc1 listed as [3, 1, 2] instead of [1, 2, 3]: another column layout, another model."""
    from pykg2vec_amd import kernels as K
    a = random_model(50, 7, 100, 50, [1, 2, 3], seed=5)
    b = random_model(50, 7, 100, 50, [3, 1, 2], seed=6)
    with torch.no_grad():
        b.load_state_dict(a.state_dict())
        for dst, src in zip(b.conv_list, (a.conv_list[2], a.conv_list[0], a.conv_list[1])):
            dst.weight.copy_(src.weight)
            dst.bias.copy_(src.bias)
    ca, cb = K.convkb_collapse(a.make_desc()), K.convkb_collapse(b.make_desc())
    assert (ca - cb).abs().max() > 1e-3 * ca.abs().max()
    A, c0 = cr.collapse64(params64(b))
    assert np.allclose(cb.double().cpu().numpy(), np.concatenate([A.reshape(-1), [c0]]), atol=300 * 2.0 ** -23 * np.abs(A).max(), rtol=0)


def bundles(rng, trip, neg, E):
    """Every positive followed by neg corruptions of its head or tail (the generator's pointwise layout)."""
    rows = np.repeat(trip, 1 + neg, 0)
    y = np.tile(np.array([1] + [-1] * neg, np.int64), len(trip))
    neg_rows = np.nonzero(y < 0)[0]
    side = rng.random(len(neg_rows)) < 0.5
    rows[neg_rows[side], 0] = rng.integers(E, size=side.sum())
    rows[neg_rows[~side], 2] = rng.integers(E, size=(~side).sum())
    return rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy(), y


def check_step_vs_float64(hip, m, E, R, batch, B, neg):
    from pykg2vec_amd.trainer import Trainer
    P = params64(m)
    loss64, g64 = cr.step64(P, *batch)
    hp = dict(hidden_size=m.hidden_size, num_filters=m.num_filters, filter_sizes=m.filter_sizes, neg_rate=neg)
    trip = np.stack(batch[:3], 1)
    cfg = hip.make_config(E, R, hp, trip, trip[:4], trip[:4], batch_size=B)
    tr = Trainer(m, cfg)
    tr.build_model()
    assert tr.step_path() == "generic"
    ids = [hip.dev(x) for x in batch]
    with torch.no_grad():
        s32 = m(*ids[:3]).double().cpu().numpy()
    e64 = cr.preds64(P, *batch[:3])
    assert np.allclose(s32, e64, rtol=1e-5, atol=1e-5 * np.abs(e64).max()), np.abs(s32 - e64).max()
    loss = tr.train_step_pointwise(*ids)
    print("loss", loss.item(), loss64)
    assert np.isclose(loss.item(), loss64, rtol=1e-5, atol=1e-6), (loss.item(), loss64)
    for key, g in zip(("ent", "rel", "fc_w", "fc_b"), tr.flat.grad_views):
        ref = np.asarray(g64[key]).reshape(tuple(g.shape))
        got = g.double().cpu().numpy()
        scale = max(1e-6, float(np.abs(ref).max()))
        err = float(np.abs(got - ref).max())
        print(key, "max abs err", err, "scale", scale)
        assert np.allclose(got, ref, atol=1e-4 * scale, rtol=1e-3), (key, err, scale)
    return tr, ids


@pytest.mark.parametrize("k,B,neg", [(100, 128, 1), (100, 4096, 1), (100, 2048, 3), (1000, 4096, 1), (1000, 2048, 3)])
def test_step_vs_float64_restatement(hip, k, B, neg):
    E, R = 3000, 40
    rng = np.random.default_rng(k + B + neg)
    m = random_model(E, R, k, 50, [1, 2], seed=k * 3 + B + neg)
    trip = np.stack([rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)], 1)
    check_step_vs_float64(hip, m, E, R, bundles(rng, trip, neg, E), B, neg)


@pytest.mark.parametrize("k,B,neg", [(100, 4096, 1), (1000, 2048, 3)])
def test_step_vs_float64_on_zipf_skewed_ids(hip, k, B, neg):
    """Hub entities and relations take most rows: their gradient rows take thousands of atomic row-adds per step."""
    E, R = 3000, 40
    rng = np.random.default_rng(k + neg)
    m = random_model(E, R, k, 50, [1, 2], seed=k + 1)
    check_step_vs_float64(hip, m, E, R, bundles(rng, skewed_triples(rng, B, E, R), neg, E), B, neg)


def test_fc1_gradients_are_bit_identical_run_to_run(hip):
    E, R, k, B, neg = 3000, 40, 100, 4096, 1
    rng = np.random.default_rng(77)
    m = random_model(E, R, k, 50, [1, 2], seed=78)
    batch = bundles(rng, skewed_triples(rng, B, E, R), neg, E)
    tr, ids = check_step_vs_float64(hip, m, E, R, batch, B, neg)
    runs = []
    for _ in range(3):
        tr.flat.grad.zero_()
        tr.train_step_pointwise(*ids)
        runs.append((tr.flat.grad_views[2].clone(), tr.flat.grad_views[3].clone()))
    for w, b in runs[1:]:
        assert torch.equal(w, runs[0][0]) and torch.equal(b, runs[0][1])
    assert runs[0][0].abs().max() > 0


@pytest.mark.parametrize("neg", [1, 3])
def test_fused_sampler_step_equals_sample_then_step(hip, neg):
    from pykg2vec_amd import kernels as K
    c = ConvCase("convkb")
    c.hp = dict(c.hp, neg_rate=neg)
    res = []
    for fused in (False, True):
        m = c.build(device="cuda")
        tr, cfg = trainer_for(hip, c, m, batch_size=64)
        assert tr._fused_pointwise_ok() and tr.step_path() == "generic"
        gen = tr._new_generator()
        tr.generator = gen
        tr.loss_buf.zero_()
        if fused:
            K.train_pointwise_logistic_sampled(tr._desc, gen.triples, gen.perm, 128, 64, neg, None, gen.slots, 11, 999, 0.0, 0, tr.loss_buf)
        else:
            b = K.sample_batch(gen.triples, gen.perm, 128, 64, neg, c.E, None, gen.slots, 11, 999, pointwise=True)
            K.train_pointwise_logistic(tr._desc, *b[:4], 0.0, 0, tr.loss_buf, bundle=1 + neg)
        res.append((K.read_loss(tr.loss_buf).item(), [g.cpu().numpy().copy() for g in tr.flat.grad_views]))
    assert np.isclose(res[0][0], res[1][0], rtol=1e-5)
    for a, b in zip(res[0][1], res[1][1]):
        assert np.abs(a).max() > 0 and np.allclose(a, b, atol=1e-6, rtol=1e-4)
    assert np.array_equal(res[0][1][2], res[1][1][2]) and np.array_equal(res[0][1][3], res[1][1][3])   # same rows, same order: same bits


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_graph_replayed_epochs_equal_eager_epochs(hip, opt):
    from pykg2vec_amd.trainer import Trainer
    c = ConvCase("convkb")
    out = []
    for use_graph in (False, True):
        cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.02, batch_size=16)
        m = c.build(device="cuda")
        tr = Trainer(m, cfg, use_graph=use_graph)
        tr.build_model()
        tr.generator = tr._new_generator()
        losses = [tr.train_model_epoch(e) for e in range(3)]
        assert (tr._graph is not None) == use_graph and tr.step_path() == "generic"
        out.append((losses, {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}))
    (l0, p0), (l1, p1) = out
    assert np.allclose(l0, l1, rtol=2e-4), (l0, l1)
    for k in TRAINED:   # rows sum under float atomics: summation order only
        assert not np.array_equal(p0[k], c.z["init." + k]), k
        assert np.allclose(p0[k], p1[k], atol=2e-4, rtol=1e-3), (k, np.abs(p0[k] - p1[k]).max())


# ---------------------------------------------------------------- ranks at FB15k size
def test_ranks_at_fb15k_size(hip):
    from pykg2vec_amd import kernels as K
    E, R, k, n = 14951, 1345, 100, 64
    rng = np.random.default_rng(91)
    m = random_model(E, R, k, 50, [1, 2], seed=92)
    trip = np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1)
    known = np.concatenate([trip, np.stack([np.repeat(trip[:, 0], 20), np.repeat(trip[:, 1], 20), rng.integers(E, size=20 * n)], 1),
                            np.stack([rng.integers(E, size=20 * n), np.repeat(trip[:, 1], 20), np.repeat(trip[:, 2], 20)], 1)])
    t_off, t_ids, h_off, h_ids = K.filter_csr_build(hip.dev(known), hip.dev(trip), E, R)
    assert t_ids.numel() > 20 * n and h_ids.numel() > 20 * n
    desc = m.make_desc()
    ranks = K.eval_ranks(desc, hip.dev(trip), t_off, t_ids, h_off, h_ids)
    tail, head = K.eval_sweep_scores_side(desc, hip.dev(trip), 0), K.eval_sweep_scores_side(desc, hip.dev(trip), 1)
    rt, frt = K.rank_from_scores(tail, hip.dev(trip[:, 2]), t_off, t_ids)
    rh, frh = K.rank_from_scores(head, hip.dev(trip[:, 0]), h_off, h_ids)
    assert torch.equal(ranks, torch.stack([rh, rt, frh, frt]))              # exactly, counted on the fp32 values the sweep stores
    assert (ranks[2] < ranks[0]).any() and (ranks[3] < ranks[1]).any()      # the filters bite
    P = params64(m)
    ents = np.arange(E)
    ranks, tail, head = ranks.cpu().numpy(), tail.cpu().numpy(), head.cpu().numpy()
    differ = 0
    for i, (h, r, t) in enumerate(trip):
        for row, row64, true, j, kn in ((tail[i], cr.preds64(P, np.full(E, h), np.full(E, r), ents), int(t), 1, known[(known[:, 0] == h) & (known[:, 1] == r), 2]),
                                        (head[i], cr.preds64(P, ents, np.full(E, r), np.full(E, t)), int(h), 0, known[(known[:, 2] == t) & (known[:, 1] == r), 0])):
            assert np.allclose(row, row64, rtol=1e-5, atol=1e-5 * np.abs(row64).max()), np.abs(row - row64).max()
            want = cr.rank64(row64, true, kn)
            for got, ref in ((ranks[j, i], want[0]), (ranks[j + 2, i], want[1])):
                ok, near = rank_band_ok(row64, true, got, ref)
                assert ok, (i, j, got, ref, near)
                differ += int(got != ref)
    print("ranks that differ from float64 (all inside the fp32 band):", differ, "of", 4 * n)


def test_trainer_and_evaluator_end_to_end(hip):
    from pykg2vec_amd.evaluator import Evaluator
    c = ConvCase("convkb")
    m = c.build(device="cuda")
    tr, cfg = trainer_for(hip, c, m, optimizer="adam", lr=0.01, batch_size=32)
    tr.generator = tr._new_generator()
    losses = [tr.train_model_epoch(e) for e in range(4)]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    metrics = Evaluator(m, cfg).test(c.test, len(c.test), epoch=0)
    assert 1.0 <= metrics["fmr"] <= c.E and 0.0 < metrics["fmrr"] <= 1.0
    # the ranks are a function of the trained tables: the float64 restatement on them agrees inside the fp32 band
    P = params64(m)
    ranks = Evaluator(m, cfg).rank_all(c.test, 8).cpu().numpy()
    for i, (h, r, t) in enumerate(c.test[:8]):
        row = cr.preds64(P, np.full(c.E, h), np.full(c.E, r), np.arange(c.E))
        ok, near = rank_band_ok(row, int(t), ranks[1, i], ko.rank_from_scores(row.astype(np.float32), int(t), set())[0])
        assert ok, (i, ranks[1, i], near)
