"""MuRP on the HIP path (csrc/kge_murp.hip): the float64 score, the hand-derived backward, the fused BCE step, the Riemannian / SGD
launch and the contracted rank sweeps against the live reference's frozen outputs (tests/golden/ref_murp*.npz) and, at the shapes
where the kernels take another path, against the long double restatement of tools/murp_reference.py; then the public Trainer /
Evaluator classes.  Tolerances: tests/test_murp_model.py derives them (TOL = 1e-10, TRAJ_TOL = 1e-8 of the array's largest value)."""
import numpy as np
import pytest
import torch

from test_murp_model import NAMES, TRAJ_TOL, batch, build, golden, known_lists, mr, near, tables, worst

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def model_with(g, tabs, rank_order=None):
    m = build(g, device="cuda")
    with torch.no_grad():
        for (_, p), a in zip(m.named_parameters(), tabs):
            p.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
    if rank_order is not None:
        m.rank_order = rank_order
    return m


def dev_batch(hip, b):
    return [hip.dev(x) for x in b]


def trainer_for(hip, g, m, optimizer="riemannian", **kw):
    from pykg2vec_amd.trainer import Trainer
    E, R = int(g["E"]), int(g["R"])
    rng = np.random.default_rng(3)
    trip = np.stack([rng.integers(E, size=300), rng.integers(R, size=300), rng.integers(E, size=300)], 1).astype(np.int64)
    hp = dict(hidden_size=int(g["k"]), neg_rate=int(g["neg_rate"]) if "neg_rate" in g.files else 3, lmbda=0.0)
    cfg = hip.make_config(E, R, hp, trip[:240], trip[240:270], trip[270:], optimizer=optimizer, lr=float(g["lr"]) if "lr" in g.files else 50.0,
                          batch_size=8, **kw)
    tr = Trainer(m, cfg)
    tr.build_model()
    return tr, cfg


def random_case(seed, E, R, k, n):
    """Tables in the live regime at any width (row norms around 0.4), a few rows outside the ball, a zero row, random bs / bo."""
    rng = np.random.default_rng(seed)
    ent = 0.4 / np.sqrt(k) * rng.standard_normal((E, k))
    rel = 0.4 / np.sqrt(k) * rng.standard_normal((R, k))
    for e in (3, E // 2, E - 1):
        ent[e] *= rng.uniform(1.2, 2.5) / np.linalg.norm(ent[e])
    rel[R - 1] *= 1.5 / np.linalg.norm(rel[R - 1])
    ent[7] = 0.0
    tabs = [rng.uniform(-1, 1, (R, k)), 0.3 * rng.standard_normal(E), 0.3 * rng.standard_normal(E), ent, rel]
    h, r, t = rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)
    h[:4], r[:4], t[:4] = (0, 7, 3, 5), (0, 1, R - 1, 2), (0, 5, 9, 7)
    y = np.where(rng.random(n) < 0.3, 1, -1)
    return tabs, (h.astype(np.int64), r.astype(np.int64), t.astype(np.int64), y.astype(np.int64))


def desc_of(tabs, grads=None, rank_order=0):
    from pykg2vec_amd import kernels as K
    R, k = tabs[0].shape
    return K.murp_desc(tabs, grads, tot_entity=tabs[1].shape[0], tot_relation=R, dim=k, rank_order=rank_order)


def to_dev(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrs]


# ---------------------------------------------------------------- the live reference's recorded outputs
@pytest.mark.parametrize("name", ["ref_murp", "ref_murp_k40"])
def test_forward_and_autograd_match_reference(hip, name):
    g = golden(name)
    m = model_with(g, tables(g, "live."))
    b = dev_batch(hip, batch(g))
    preds = m(b[0], b[1], b[2])
    assert preds.dtype == torch.float64
    print("preds", worst(preds.detach().cpu().numpy(), g["step.preds"]))
    assert near(preds.detach().cpu().numpy(), g["step.preds"])
    loss = m.loss(preds, b[3].double())
    loss.backward()
    assert near(loss.item(), g["step.loss"])
    for n, p in m.named_parameters():
        got = p.grad.cpu().numpy()
        print(n, worst(got, g["step.grad." + n]))
        assert near(got, g["step.grad." + n]), (n, worst(got, g["step.grad." + n]))
    assert not m.ent_embeddings.weight.grad[0].any() and not m.rel_embeddings.weight.grad[0].any()    # padding_idx = 0
    assert m.wu.grad[0].any() and m.bs.grad[0] != 0 and m.bo.grad[0] != 0


@pytest.mark.parametrize("name", ["ref_murp", "ref_murp_k40"])
@pytest.mark.parametrize("opt", ["riemannian", "sgd"])
def test_fused_step_and_optimiser_match_reference(hip, name, opt):
    g = golden(name)
    m = model_with(g, tables(g, "live."))
    tr, _ = trainer_for(hip, g, m, optimizer=opt)
    assert tr.flat.param.dtype == torch.float64 and tr.loss_buf.dtype == torch.float64 and tr.step_path() == "murp"
    loss = tr.train_step_pointwise(*dev_batch(hip, batch(g)))
    assert loss.dtype == torch.float64 and near(loss.item(), g["step.loss"])
    for n, gv in zip(NAMES, tr.flat.grad_views):
        assert near(gv.cpu().numpy(), g["step.grad." + n]), (n, worst(gv.cpu().numpy(), g["step.grad." + n]))
    untouched = ~tr.flat.grad_views[3].any(1).cpu().numpy()
    tr._reduce_and_step()
    assert not tr.flat.grad.any()                             # the launch cleared what it consumed
    sd = m.state_dict()
    for n in NAMES:
        want = g["step.%s.%s" % (opt, n)]
        assert sd[n].dtype == torch.float64 and near(sd[n].cpu().numpy(), want), (n, worst(sd[n].cpu().numpy(), want))
    assert untouched.any()
    assert np.array_equal(sd["ent_embeddings.weight"].cpu().numpy()[untouched], g["live.ent_embeddings.weight"][untouched])


def test_saturated_rows_give_exact_zeros_and_a_zero_row_stays_finite(hip):
    from pykg2vec_amd import kernels as K
    g = golden("ref_murp")
    sat = g["batch.saturated"]
    h, r, t, _ = batch(g)
    tabs = to_dev(tables(g, "live."))
    grads = [torch.zeros_like(a) for a in tabs]
    K.murp_score_backward(desc_of(tabs, grads), hip.dev(h[sat]), hip.dev(r[sat]), hip.dev(t[sat]), torch.ones(int(sat.sum()), dtype=torch.float64).cuda())
    assert not grads[0].any() and not grads[3].any() and not grads[4].any() and grads[1].any() and grads[2].any()
    host = [a.copy() for a in tables(g, "live.")]
    host[3][9] = 0.0
    host[4][2] = 0.0
    hh, rr, tt = np.array([9, 4, 9]), np.array([2, 2, 1]), np.array([4, 9, 9])
    tabs = to_dev(host)
    grads = [torch.zeros_like(a) for a in tabs]
    d = desc_of(tabs, grads)
    preds = K.murp_score_forward(d, hip.dev(hh), hip.dev(rr), hip.dev(tt))
    K.murp_score_backward(d, hip.dev(hh), hip.dev(rr), hip.dev(tt), torch.ones(3, dtype=torch.float64).cuda())
    assert torch.isfinite(preds).all() and all(torch.isfinite(a).all() for a in grads)
    assert near(preds.cpu().numpy(), mr.forward(host, hh, rr, tt))
    for a, w in zip(grads, mr.backward(host, hh, rr, tt, np.ones(3))):
        assert near(a.cpu().numpy(), w)


def test_trajectory_matches_reference(hip):
    g = golden("ref_murp")
    m = model_with(g, tables(g, "init."))
    tr, _ = trainer_for(hip, g, m)
    for i in range(4):
        loss = tr.train_step_pointwise(*dev_batch(hip, batch(g, "traj.batch%d." % i)))
        assert near(loss.item(), g["traj.loss"][i], TRAJ_TOL), (i, loss.item(), g["traj.loss"][i])
        tr._reduce_and_step()
    sd = m.state_dict()
    for n in NAMES:
        print(n, worst(sd[n].cpu().numpy(), g["traj.after." + n]))
        assert near(sd[n].cpu().numpy(), g["traj.after." + n], TRAJ_TOL), (n, worst(sd[n].cpu().numpy(), g["traj.after." + n]))


def test_rank_lists_and_ranks_match_reference(hip):
    """predict_*_rank return the reference's lists; eval_ranks with rank_order = 0 gives the true entity's position in them, with
    rank_order = 1 the reference MetricCalculator's raw and filtered ranks; no ties anywhere in this fixture."""
    from pykg2vec_amd import kernels as K
    g = golden("ref_murp")
    E, R = int(g["E"]), int(g["R"])
    q = hip.dev(g["eval.queries"])
    csr = K.filter_csr_build(hip.dev(g["eval.known"]), q, E, R)
    m = model_with(g, tables(g, "live."))
    for i in (0, 1, 17, 39):
        h, r, t = (q[i, j].view(1) for j in range(3))
        assert np.array_equal(m.predict_tail_rank(h, r, topk=5).cpu().numpy(), g["eval.tail_list"][i])
        assert np.array_equal(m.predict_head_rank(t, r, topk=5).cpu().numpy(), g["eval.head_list"][i])
    ties = torch.zeros((2, q.shape[0]), dtype=torch.int32, device=q.device)
    ranks = K.eval_ranks(m.make_desc(), q, *csr, ties=ties).cpu().numpy()
    assert np.array_equal(ranks[0], g["eval.pos_head"]) and np.array_equal(ranks[1], g["eval.pos_tail"])
    assert not ties.any()
    m.rank_order = 1
    ranks = K.eval_ranks(m.make_desc(), q, *csr, ties=ties).cpu().numpy()
    for row, key in enumerate(("rank_head", "rank_tail", "frank_head", "frank_tail")):
        assert np.array_equal(ranks[row], g["eval." + key]), key
    assert not ties.any()
    i = 17
    assert np.array_equal(m.predict_tail_rank(q[i, 0].view(1), q[i, 1].view(1)).cpu().numpy(), g["eval.tail_list"][i][::-1])
    # relation ranking through the batch scorer
    h, r, t = (int(x) for x in g["eval.queries"][5])
    want = mr.forward(tables(g, "live."), np.full(R, h), np.arange(R), np.full(R, t))
    m.rank_order = 0
    assert np.array_equal(m.predict_rel_rank(q[5, 0].view(1), q[5, 2].view(1), topk=3).cpu().numpy(), np.argsort(want, kind="stable"))


def test_tie_band(hip):
    """bs = bo = 0 and a third of the rows outside the ball: saturated candidates tie bit for bit, the counts are exact with respect
    to the stored sweep scores, and the reference's list position lies inside the tie band."""
    from pykg2vec_amd import kernels as K
    g = golden("ref_murp_ties")
    q = hip.dev(g["eval.queries"])
    m = model_with(g, tables(g, "live."))
    csr = K.filter_csr_build(hip.dev(g["eval.known"]), q, int(g["E"]), int(g["R"]))
    for order in (0, 1):
        m.rank_order = order
        d = m.make_desc()
        ties = torch.zeros((2, q.shape[0]), dtype=torch.int32, device=q.device)
        ranks = K.eval_ranks(d, q, *csr, ties=ties).cpu().numpy()
        ties = ties.cpu().numpy()
        assert ties.sum() > 0
        for side, col, row in ((0, 2, 1), (1, 0, 0)):
            s = K.eval_sweep_scores_side(d, q, side).cpu().numpy()
            for i, trip in enumerate(g["eval.queries"]):
                kt, kh = known_lists(g, *trip)
                want = mr.ranks(s[i], trip[col], kh if side else kt, order)
                assert (ranks[row][i], ranks[row + 2][i], ties[row][i]) == want, (order, side, i)
        if order == 0:
            assert np.all((ranks[1] <= g["eval.pos_tail"]) & (g["eval.pos_tail"] <= ranks[1] + ties[1]))
            assert np.all((ranks[0] <= g["eval.pos_head"]) & (g["eval.pos_head"] <= ranks[0] + ties[0]))


# ---------------------------------------------------------------- every lane-group geometry, more than one workgroup and tile
# k: the edges of (16, 1) (16, 3) (64, 2) (64, 8) (64, 32) columns per lane; E = 131: three candidate tiles, the last one of 3;
# 37 queries: three query tiles; 301 rows: more than one workgroup at every group width
@pytest.mark.parametrize("k", [1, 7, 16, 17, 40, 48, 49, 128, 129, 512, 513])
def test_step_and_sweeps_vs_long_double(hip, k):
    from pykg2vec_amd import kernels as K
    E, R, n, nq = 131, 5, 301, 37
    host, (h, r, t, y) = random_case(100 + k, E, R, k, n)
    preds_w, loss_w, grads_w = mr.train_bce(host, h, r, t, y, dtype=np.longdouble)
    tabs = to_dev(host)
    grads = [torch.zeros_like(a) for a in tabs]
    d = desc_of(tabs, grads)
    ids = [hip.dev(x) for x in (h, r, t, y)]
    preds = K.murp_score_forward(d, *ids[:3]).cpu().numpy()
    print("k", k, "preds", worst(preds, preds_w))
    assert near(preds, preds_w), worst(preds, preds_w)
    loss = K.murp_new_loss("cuda")
    K.murp_train_bce(d, *ids, loss)
    assert near(loss.item(), loss_w)
    for a, w, name in zip(grads, grads_w, NAMES):
        print("   ", name, worst(a.cpu().numpy(), w))
        assert near(a.cpu().numpy(), w), (name, worst(a.cpu().numpy(), w))
    new_w = mr.rsgd_step(host, grads_w, 50.0, True, np.longdouble)
    K.murp_rsgd_step(d, 50.0, riemannian=True)
    assert not any(a.any() for a in grads)
    for a, w, name in zip(tabs, new_w, NAMES):
        assert near(a.cpu().numpy(), w), ("rsgd", name, worst(a.cpu().numpy(), w))
    # sweeps on the original tables
    tabs = to_dev(host)
    d = desc_of(tabs)
    q = np.stack([h[:nq], r[:nq], t[:nq]], 1)
    for side in (0, 1):
        s = K.murp_sweep_scores_side(d, hip.dev(q), side).cpu().numpy()
        for i in (0, 1, 2, 3, 16, nq - 1):
            want = mr.sweep_tail(host, q[i, 0], q[i, 1], np.longdouble) if side == 0 else mr.sweep_head(host, q[i, 1], q[i, 2], np.longdouble)
            assert near(s[i], want), (side, i, worst(s[i], want))
    ties = torch.zeros((2, nq), dtype=torch.int32).cuda()
    ranks = K.eval_ranks(d, hip.dev(q), None, None, None, None, ties=ties).cpu().numpy()
    st, sh = K.murp_sweep_scores_side(d, hip.dev(q), 0).cpu().numpy(), K.murp_sweep_scores_side(d, hip.dev(q), 1).cpu().numpy()
    for i in range(nq):
        assert (ranks[1][i], ranks[3][i]) == mr.ranks(st[i], q[i, 2])[:2] and (ranks[0][i], ranks[2][i]) == mr.ranks(sh[i], q[i, 0])[:2]


def test_opcheck_murp_score(hip):
    from pykg2vec_amd import ops
    g = golden("ref_murp")
    m = model_with(g, tables(g, "live."))
    h, r, t = dev_batch(hip, batch(g))[:3]
    weights = m.trainable_tensors()
    key = ops.register_model(m)
    # (the static checks: the backward's float64 atomics make two real runs differ in the last bits)
    torch.library.opcheck(torch.ops.kge.murp_score.default, (key, h, r, t, weights),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    got = torch.ops.kge.murp_score(key, h, r, t, weights)
    assert got.shape == (h.numel(),) and got.dtype == torch.float64 and got.requires_grad and torch.equal(got, m(h, r, t))


def test_debug_mode_refuses_an_id_out_of_range(hip):
    from pykg2vec_amd import kernels as K
    g = golden("ref_murp")
    d = desc_of(to_dev(tables(g, "live.")))
    ids = hip.dev(np.array([1, 2, int(g["E"])]))
    K.set_debug(True)
    try:
        with pytest.raises(K.L.KgeHipError):
            K.murp_score_forward(d, ids, hip.dev(np.zeros(3, np.int64)), hip.dev(np.zeros(3, np.int64)))
    finally:
        K.set_debug(False)


# ---------------------------------------------------------------- the public classes
def test_trainer_and_evaluator_end_to_end(hip, tmp_path):
    g = golden("ref_murp")
    m = build(g, device="cuda")
    tr, cfg = trainer_for(hip, g, m, path_tmp=str(tmp_path))
    tr.generator = tr._new_generator()
    losses = [tr.train_model_epoch(e) for e in range(3)]
    assert tr.step_path() == "murp" and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(p.dtype == torch.float64 and torch.isfinite(p).all() for p in m.parameters())
    tr.evaluator.test(tr.evaluator.test_data, 20)
    assert tr.evaluator.tie_counts is not None and tr.evaluator.tie_counts.shape == (2, 20) and (tr.evaluator.tie_counts >= 0).all()
    assert tr.evaluator.test_rel_rank(1, 2).shape == (cfg.tot_relation,) and tr.evaluator.test_tail_rank(1, 2).shape == (cfg.tot_entity,)
    tr.save_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    state = torch.load(str(tmp_path / "murp" / "model.vec.pt"))
    assert tuple(state.keys()) == NAMES and all(v.dtype == torch.float64 for v in state.values())
    tr.flat.param.zero_()
    tr.load_model()
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
