"""KG2E (generic row kernels, csrc/kge_device.h) and HoLE (csrc/kge_hole.hip) on the HIP path: parity with the frozen reference
outputs in tests/golden/ref_{kg2e,kg2e_clip,hole}.npz, larger shapes against a float64 torch restatement of the reference's
forward, the fused-sampler step, hipGraph replay, and the rank sweeps (csrc/kge_kg2e_eval.hip, the negated-dot pipeline)."""
import numpy as np
import pytest
import torch

import kge_oracle as ko
from golden_util import Case, close, rank_band_ok

pytestmark = pytest.mark.gpu

NAMES = ["kg2e", "kg2e_clip", "hole"]
GRAD_TOL = dict(atol=2e-5, rtol=1e-4)


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def case(name):
    c = Case(name)
    c.model = "kg2e" if name.startswith("kg2e") else name   # kg2e_clip: KG2E with un-swapped clip settings
    return c


# ---------------------------------------------------------------- float64 restatements of pairwise.py:1035-1142
def hole_basis(d):
    jk = torch.outer(torch.arange(d), torch.arange(d)) % d
    return torch.cos(2 * np.pi * jk.double() / d), torch.sin(2 * np.pi * jk.double() / d)


def energy64(model, P, h, r, t):
    if model == "kg2e":
        nz = lambda x: x / x.norm(dim=-1, keepdim=True)
        hm, hs = nz(P["ent_embeddings_mu"][h]), nz(P["ent_embeddings_sigma"][h])
        rm, rs = nz(P["rel_embeddings_mu"][r]), nz(P["rel_embeddings_sigma"][r])
        tm, ts = nz(P["ent_embeddings_mu"][t]), nz(P["ent_embeddings_sigma"][t])
        cs, cm = hs + rs, hm + rm
        return (cs / ts).sum(-1) + ((tm - cm) ** 2 / ts).sum(-1) + (torch.log(ts) - torch.log(cs)).sum(-1) - hm.shape[1]
    eh, et = P["ent_embeddings"][h], P["ent_embeddings"][t]
    rr = torch.nn.functional.normalize(P["rel_embeddings"][r], p=2, dim=-1)
    C, S = hole_basis(eh.shape[1])
    x = ((eh @ C) * (et @ C) * (rr @ C) - (eh @ S) * (et @ S) * (rr @ S)).sum(1) / eh.shape[1]
    return -torch.sigmoid(x)


def random_case(hip, model, E, R, d, seed):
    rng = np.random.default_rng(seed)
    hp = dict(hidden_size=d, cmax=5.0, cmin=0.05, margin=1.0)   # KG2E: sigma = xavier + 1 > 0, rows of varying norm
    torch.manual_seed(seed)
    m = hip.model_from_params(model, {}, hp, E, R)
    with torch.no_grad():   # entity rows of different lengths: the normalisation backward is exercised
        for p in m.parameter_list:
            if p.weight.shape[0] == E:
                p.weight.mul_(torch.from_numpy(rng.uniform(0.5, 2.0, (E, 1)).astype(np.float32)).to(p.weight.device))
    return m, hp


def batch_of(rng, E, R, B):
    pos = np.stack([rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)], 1)
    neg = pos.copy()
    side = rng.random(B) < 0.5
    neg[side, 0] = rng.integers(E, size=side.sum())
    neg[~side, 2] = rng.integers(E, size=(~side).sum())
    return (pos[:, 0], pos[:, 1], pos[:, 2], neg[:, 0], neg[:, 1], neg[:, 2])


# ---------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_reference_golden(hip, name):
    c = case(name)
    m = hip.model_from_case(c)
    b = c.batch(0)
    with torch.no_grad():
        gp = m(hip.dev(b[0]), hip.dev(b[1]), hip.dev(b[2])).cpu().numpy()
        gn = m(hip.dev(b[3]), hip.dev(b[4]), hip.dev(b[5])).cpu().numpy()
    assert close(gp, c.z["scores0_pos"], atol=2e-5, rtol=2e-5), np.abs(gp - c.z["scores0_pos"]).max()
    assert close(gn, c.z["scores0_neg"], atol=2e-5, rtol=2e-5), np.abs(gn - c.z["scores0_neg"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_autograd_path_matches_reference_grads(hip, name):
    c = case(name)
    m = hip.model_from_case(c)
    b = [hip.dev(x) for x in c.batch(0)]
    m.train()
    loss = m.loss(m(b[0], b[1], b[2]), m(b[3], b[4], b[5]), c.hp["margin"])
    loss.backward()
    assert close(loss.item(), c.z["loss0"], atol=2e-5, rtol=2e-5), (loss.item(), c.z["loss0"])
    for k, p in hip.table_parameters(m):
        ref = c.z["grad0." + k]
        got = p.grad.cpu().numpy()
        assert np.allclose(got, ref, **GRAD_TOL), (k, np.abs(got - ref).max())


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_matches_reference_loss_and_grads(hip, name):
    from pykg2vec_amd.trainer import Trainer
    c = case(name)
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    m = hip.model_from_case(c)
    tr = Trainer(m, cfg)
    tr.build_model()
    assert tr.step_path() == "generic" and tr._fused_sampler_ok() == (c.model == "kg2e")
    loss = tr.train_step_pairwise(*[hip.dev(x) for x in c.batch(0)])
    assert close(loss.item(), c.z["loss0"], atol=2e-5, rtol=2e-5), (loss.item(), c.z["loss0"])
    for (k, _), g in zip(hip.table_parameters(m), tr.flat.grad_views):
        ref = c.z["grad0." + k]
        assert np.allclose(g.cpu().numpy(), ref, **GRAD_TOL), (k, np.abs(g.cpu().numpy() - ref).max())


def replay64(c, opt):
    """The reference's three optimiser steps (utils/trainer.py:112-131, torch.optim defaults) in float64."""
    P = {k[len("init."):-len(".weight")]: torch.tensor(c.z[k], dtype=torch.float64, requires_grad=True)
         for k in c.z.files if k.startswith("init.")}
    cls = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adagrad": torch.optim.Adagrad, "rms": torch.optim.RMSprop}[opt]
    o = cls(list(P.values()), lr=0.05)
    for s in range(3):
        b = [torch.as_tensor(x) for x in c.batch(s)]
        o.zero_grad()
        torch.sum(torch.clamp(energy64(c.model, P, *b[:3]) + c.hp["margin"] - energy64(c.model, P, *b[3:]), min=0)).backward()
        o.step()
    return {k + ".weight": v.detach().numpy() for k, v in P.items()}


# kg2e_clip under RMSprop at lr 0.05 diverges in the reference (losses 68.6, 229.5, NaN): updates of +-0.5 per entry per step
# make its final weights a function of rounding residues, so that pair has no usable final-weight yardstick
@pytest.mark.parametrize("name,opt", [(n, o) for n in NAMES for o in ("sgd", "adam", "adagrad", "rms") if (n, o) != ("kg2e_clip", "rms")])
def test_three_fused_training_steps_match_reference_weights(hip, name, opt):
    from pykg2vec_amd.trainer import Trainer
    c = case(name)
    cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.05)
    m = hip.model_from_case(c)
    tr = Trainer(m, cfg)
    tr.build_model()
    losses = []
    for s in range(3):
        losses.append(tr.train_step_pairwise(*[hip.dev(x) for x in c.batch(s)]).item())
        tr._reduce_and_step()
    assert close(np.asarray(losses), c.z["%s.losses" % opt], atol=3e-5, rtol=3e-5), (losses, c.z["%s.losses" % opt])
    # KG2E's default init (every sigma entry 5.0) makes the sigma gradient of head / relation rows zero in exact arithmetic; an
    # fp32 implementation leaves a rounding residue there (the reference's autograd and these kernels, each its own), and Adam /
    # Adagrad / RMSprop scale a residue up to about lr.  An entry must agree with the fp32 reference OR with the same three steps
    # in float64 (replay64; the reference itself differs from float64 by up to 0.12 there); the few that follow this
    # implementation's own residues must stay within three steps' reach of their initial value.
    r64 = replay64(c, opt) if c.model == "kg2e" and opt != "sgd" else None
    tol = 2e-3 if opt == "rms" else 1e-4
    for k, p in hip.table_parameters(m):
        ref = c.z["%s.final.%s" % (opt, k)]
        got = p.detach().cpu().numpy()
        bad = ~np.isclose(got, ref, atol=tol, rtol=1e-4)
        if r64 is not None:
            bad &= ~np.isclose(got, r64[k], atol=tol, rtol=1e-4)
            reach = 3 * 0.05 * (10 if opt == "rms" else 1) + tol   # three steps of at most lr (RMSprop: lr / sqrt(1 - alpha))
            assert np.all(np.abs(got - c.z["init." + k])[bad] <= reach), k
            assert bad.mean() <= 0.1, (k, bad.sum(), np.abs(got - ref).max())
            continue
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
    with torch.no_grad():   # the sweep's energies are the forward's, to fp32 rounding
        E = c.E
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


# ---------------------------------------------------------------- larger shapes against float64
SHAPES = [(model, d, B) for model in ("kg2e", "hole") for d in (50, 100, 150) for B in (128, 4096, 50000)]


@pytest.mark.parametrize("model,d,B", SHAPES)
def test_step_vs_float64_restatement(hip, model, d, B):
    check_step_vs_float64(hip, model, 3000, 40, d, B, seed=d * 7 + B)


def check_step_vs_float64(hip, model, E, R, d, B, seed):
    """Forward energies and one fused step of a random model against the float64 restatement (energy64 + autograd)."""
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    m, hp = random_case(hip, model, E, R, d, seed=seed)
    batch = batch_of(np.random.default_rng(B + d), E, R, B)
    desc = m.make_desc()
    with torch.no_grad():
        sp = K.score_forward(desc, *[hip.dev(x) for x in batch[:3]]).cpu().double()
        sn = K.score_forward(desc, *[hip.dev(x) for x in batch[3:]]).cpu().double()
    P = {k.split(".")[0]: p.detach().cpu().double().requires_grad_(True) for k, p in hip.table_parameters(m)}
    ids = [torch.as_tensor(x) for x in batch]
    ep, en = energy64(model, P, *ids[:3]), energy64(model, P, *ids[3:])
    for got, want in ((sp, ep), (sn, en)):
        assert torch.allclose(got, want.detach(), rtol=1e-5, atol=1e-5 * float(want.detach().abs().max())), (got - want).abs().max()
    coeff = ((sp + hp["margin"] - sn) > 0).double()   # the hinge mask of OUR fp32 energies
    loss64 = torch.sum(torch.clamp(ep + hp["margin"] - en, min=0) * coeff)
    torch.sum(coeff * (ep - en)).backward()
    cfg = hip.make_config(E, R, hp, np.stack(batch[:3], 1), np.stack(batch[:3], 1)[:4], np.stack(batch[:3], 1)[:4], batch_size=B)
    tr = Trainer(m, cfg)
    tr.build_model()
    loss = tr.train_step_pairwise(*[hip.dev(x) for x in batch])
    assert np.isclose(loss.item(), loss64.item(), rtol=1e-5, atol=1e-5), (loss.item(), loss64.item())
    for (k, _), g in zip(hip.table_parameters(m), tr.flat.grad_views):
        ref = P[k.split(".")[0]].grad.numpy()
        got = g.cpu().numpy()
        scale = max(1e-3, np.abs(ref).max())
        assert np.allclose(got, ref, atol=1e-4 * scale, rtol=1e-3), (k, np.abs(got - ref).max(), scale)


def test_kg2e_fused_sampler_step_equals_sample_then_step(hip):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    for name in ("kg2e", "kg2e_clip"):
        c = case(name)
        cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, batch_size=64)
        res = []
        for fused in (False, True):
            m = hip.model_from_case(c)
            tr = Trainer(m, cfg)
            tr.build_model()
            assert tr._fused_sampler_ok()
            gen = tr._new_generator()
            tr.generator = gen
            tr.loss_buf.zero_()
            if fused:
                K.train_pairwise_hinge_sampled(tr._desc, gen.triples, gen.perm, 128, 64, None, gen.slots, 11, 999, 1.0, tr.loss_buf)
            else:
                b = K.sample_batch(gen.triples, gen.perm, 128, 64, 1, c.E, None, gen.slots, 11, 999)
                K.train_pairwise_hinge(tr._desc, *b, 1.0, tr.loss_buf)
            res.append((K.read_loss(tr.loss_buf).item(), [g.cpu().numpy().copy() for g in tr.flat.grad_views]))
        assert np.isclose(res[0][0], res[1][0], rtol=1e-5)
        for a, b in zip(res[0][1], res[1][1]):
            assert np.allclose(a, b, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("name,opt", [("kg2e", "adam"), ("kg2e_clip", "sgd"), ("hole", "adagrad")])
def test_graph_replayed_epochs_equal_eager_epochs(hip, name, opt):
    from pykg2vec_amd.trainer import Trainer
    c = case(name)
    out = []
    for use_graph in (False, True):
        cfg = hip.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, optimizer=opt, lr=0.02, batch_size=16)
        m = hip.model_from_case(c)
        tr = Trainer(m, cfg, use_graph=use_graph)
        tr.build_model()
        tr.generator = tr._new_generator()
        losses = [tr.train_model_epoch(e) for e in range(3)]
        assert (tr._graph is not None) == use_graph
        out.append((losses, {k: p.detach().cpu().numpy() for k, p in hip.table_parameters(m)}))
    (l0, p0), (l1, p1) = out
    assert np.allclose(l0, l1, rtol=2e-4), (l0, l1)
    for k in p0:   # rows sum under float atomics: summation order only
        assert np.allclose(p0[k], p1[k], atol=2e-4, rtol=1e-3), (k, np.abs(p0[k] - p1[k]).max())


def test_hole_matrix_core_sweep_and_small_query_sweep_agree(hip, monkeypatch):
    """>= 512 query rows go to k_eval_gemm; KGE_EVAL_GEMM=0 forces the VALU sweep.  Ranks agree except at fp32 near-ties."""
    from pykg2vec_amd import kernels as K
    E, R, d, n = 3000, 40, 50, 600
    m, _ = random_case(hip, "hole", E, R, d, seed=11)
    rng = np.random.default_rng(12)
    trips = hip.dev(np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1))
    out = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("KGE_EVAL_GEMM", sw)
        out[sw] = (K.eval_ranks(m.make_desc(), trips, None, None, None, None).cpu().numpy(),
                   K.eval_sweep_scores(m.make_desc(), trips).cpu().numpy())
    (r1, s1), (r0, s0) = out["1"], out["0"]
    assert np.allclose(s1, s0, atol=1e-6, rtol=1e-5)
    tn = trips.cpu().numpy()
    for i in range(n):
        for row, true, a in ((s0[2 * i], tn[i, 2], 1), (s0[2 * i + 1], tn[i, 0], 0)):
            ok, near = rank_band_ok(row, int(true), r1[a, i], r0[a, i])
            assert ok, (i, a, r1[a, i], r0[a, i], near)
    assert (r1 != r0).sum() <= 0.01 * r1.size


@pytest.mark.parametrize("gemm", ["1", "0"])
def test_hole_saturated_ties_rank_like_the_reference(hip, monkeypatch, gemm):
    """Logits scaled past +-20: the reference's fp32 sigmoid saturates to -1.0 (ties).  Ranks come from -sigmoid(x), not from x,
    so they equal kge_oracle.rank_from_scores on a float32 torch restatement of the reference's forward."""
    from pykg2vec_amd import kernels as K
    E, R, d, n = 700, 5, 16, 300
    m, _ = random_case(hip, "hole", E, R, d, seed=21)
    with torch.no_grad():
        m.ent_embeddings.weight.mul_(200.0)   # |x| in the hundreds: about half the candidates saturate to -1.0
    monkeypatch.setenv("KGE_EVAL_GEMM", gemm)
    rng = np.random.default_rng(22)
    trips = np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1)
    ranks = K.eval_ranks(m.make_desc(), hip.dev(trips), None, None, None, None).cpu().numpy()
    ent = m.ent_embeddings.weight.detach().cpu()
    rel = m.rel_embeddings.weight.detach().cpu()
    C, S = (x.float() for x in hole_basis(d))
    ce, se = ent @ C, ent @ S
    saturated, off = 0, 0
    for i, (h, r, t) in enumerate(trips):
        rr = torch.nn.functional.normalize(rel[r:r + 1], p=2, dim=-1)
        cr, sr = rr @ C, rr @ S
        xt = ((ce[h:h + 1] * cr) * ce - (se[h:h + 1] * sr) * se).sum(1) / d     # tail sweep (h, r, e)
        xh = (ce * (ce[t:t + 1] * cr) - se * (se[t:t + 1] * sr)).sum(1) / d     # head sweep (e, r, t)
        for x, true, got in ((xt, int(t), ranks[1, i]), (xh, int(h), ranks[0, i])):
            s32 = (-torch.sigmoid(x)).numpy()
            want = ko.rank_from_scores(s32, true, set())[0]
            if s32[true] == -1.0:   # the true candidate sits in a saturated tie: exact (ranking on x would count the others)
                saturated += 1
                assert got == want == 0, (i, got, want, int((x > x[true]).sum()))
            else:                   # unsaturated: fp32 rounding of x may reorder a near-tie
                off += int(got != want)
                assert abs(int(got) - want) <= 2, (i, got, want)
    assert saturated > n // 4, saturated   # the ties are really there
    assert off <= 0.01 * 2 * n, off
