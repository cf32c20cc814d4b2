"""TuckER on the HIP path (csrc/kge_tucker.hip): parity with the reference's float64 outputs in tests/golden/ref_tucker{,_ls}.npz
(exact ranks), edge shapes and a production-size step against the float64 restatement of tools/tucker_reference.py with shared Philox
masks, the ordered core gradient, the autograd path and the public Trainer / Evaluator classes.

Tolerances: on every test shape the plain fp32 numpy run of the same formulas (tucker_reference.step(dtype=np.float32)) is compared
with the float64 one; the HIP path is allowed FACTOR = 4 times that error per quantity (predictions, loss, each gradient relative to
its max-abs), the factor covering another summation order on the matrix cores and in the atomics.  The errors are measured where
they are used (`bounds`), printed, and floored at one fp32 ulp of the quantity (2^-23 relative): a measured error of zero cannot be a
bound.  DESIGN.md section 15 lists the figures of these shapes."""
import numpy as np
import pytest
import torch

from test_tucker_model import NAMES, TABLES, fixture, tables, tr

pytestmark = pytest.mark.gpu
FACTOR = 4.0
ULP = 2.0 ** -23
DROP = (0.3, 0.4, 0.5)


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    """A Trainer reads the KGE_* A/B switches from the process environment, and other test modules of this suite leave some of them
    set (tests/test_hip_dist.py writes os.environ directly): every test here starts without them."""
    from test_tucker_model import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def csr(y):
    off = np.concatenate([[0], np.cumsum((y != 0).sum(1))]).astype(np.int64)
    ids = np.concatenate([np.flatnonzero(row) for row in y] + [np.zeros(0, np.int64)]).astype(np.int32)
    return torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda()


def model_for(P, dropouts=(0.0, 0.0, 0.0)):
    from pykg2vec_amd.projection import TuckER
    E, d1 = P[TABLES[0]].shape
    R, d2 = P[TABLES[1]].shape
    m = TuckER(tot_entity=E, tot_relation=R, ent_hidden_size=d1, rel_hidden_size=d2, lmbda=0.0, input_dropout=dropouts[0],
               hidden_dropout1=dropouts[1], hidden_dropout2=dropouts[2])
    m.load_state_dict({k: torch.from_numpy(np.asarray(P[k], dtype=np.float32)) for k in TABLES})
    return m.cuda()


def fused(P, h, r, t, y1, y2, dropouts=(0.0, 0.0, 0.0), seed=0, offset=0, ls=None):
    """(loss, {table: gradient}) of kge_tucker_train_bce."""
    from pykg2vec_amd import kernels as K
    m = model_for(P, dropouts)
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=seed, offset=offset)
    loss = K.new_loss_buffer(ws[0].device)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()
    K.tucker_train_bce(d, dev(h), dev(r), dev(t), *csr(y1), *csr(y2), ls, loss)
    return K.read_loss(loss).item(), {k: g.cpu().numpy().astype(np.float64) for k, g in zip(TABLES, gs)}


def bounds(P, h, r, t, y1, y2, **kw):
    """float64 results and FACTOR x the fp32 restatement's error per quantity."""
    ref = tr.step(P, h, r, t, y1, y2, **kw)
    f32 = tr.step(P, h, r, t, y1, y2, dtype=np.float32, **kw)
    b = {"loss": FACTOR * max(abs(f32[0] - ref[0]), ULP * abs(ref[0])),
         "preds": FACTOR * max(np.abs(f32[2] - ref[2]).max(), np.abs(f32[3] - ref[3]).max(), ULP)}
    for k in TABLES:
        b[k] = FACTOR * max(np.abs(f32[1][k] - ref[1][k]).max(), ULP * np.abs(ref[1][k]).max())
    return ref, b


def check_step(tag, got, ref, b):
    loss, g = got
    print(tag, "loss err %.3g (bound %.3g)" % (abs(loss - ref[0]), b["loss"]))
    bad = [] if abs(loss - ref[0]) <= b["loss"] else ["loss"]
    for k in TABLES:
        err = np.abs(g[k] - ref[1][k]).max()
        print(tag, k, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[k], np.abs(ref[1][k]).max()))
        if not err <= b[k]:
            bad.append(k)
    assert not bad, (tag, bad)


# ---------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_fixture_parity(hip, name):
    from pykg2vec_amd import kernels as K
    z = fixture(name)
    P = tables(z)
    ref, b = bounds(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], label_smoothing=z["ls"])
    m = model_for(P)
    m.eval()
    with torch.no_grad():
        pt = m(hip.dev(z["h"]), hip.dev(z["r"]), direction="tail").cpu().numpy()
        ph = m(hip.dev(z["t"]), hip.dev(z["r"]), direction="head").cpu().numpy()
    err = max(np.abs(pt - z["pred_tails"]).max(), np.abs(ph - z["pred_heads"]).max())
    print(name, "preds err %.3g (bound %.3g)" % (err, b["preds"]))
    assert err <= b["preds"]
    want = (float(z["loss"]), {k: z["grad." + k] for k in TABLES})
    check_step(name, fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], ls=z["ls"]), want, b)
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    trip = hip.dev(z["test"])
    t_off, t_ids, h_off, h_ids = K.filter_csr_build(hip.dev(known), trip, int(z["E"]), int(z["R"]))
    ties = torch.zeros((2, len(z["test"])), dtype=torch.int32, device="cuda")
    ranks = K.tucker_eval_ranks(m.make_desc(), trip, t_off, t_ids, h_off, h_ids, ties=ties).cpu().numpy()
    assert np.array_equal(ranks, z["ranks"]), (ranks, z["ranks"])    # exact, all of them
    assert int(ties.sum()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_rank_pass_with_one_side_unfiltered_and_with_one_triple(hip, name):
    """The shared rank pass (csrc/kge_projection.hip) with an absent filter on either side and with n = 1: exact against the ranks
    the reference recorded."""
    from pykg2vec_amd import kernels as K
    z = fixture(name)
    desc = model_for(tables(z)).make_desc(train=False)
    known = hip.dev(np.concatenate([z["train"], z["valid"], z["test"]]))
    trip = hip.dev(z["test"])
    t_off, t_ids, h_off, h_ids = K.filter_csr_build(known, trip, int(z["E"]), int(z["R"]))
    want = z["ranks"]      # rows: head, tail, filtered head, filtered tail
    got = K.eval_ranks(desc, trip, None, None, h_off, h_ids).cpu().numpy()
    assert np.array_equal(got[0:2], want[0:2]) and np.array_equal(got[3], got[1]) and np.array_equal(got[2], want[2]), (got, want)
    got = K.eval_ranks(desc, trip, t_off, t_ids, None, None).cpu().numpy()
    assert np.array_equal(got[0:2], want[0:2]) and np.array_equal(got[2], got[0]) and np.array_equal(got[3], want[3]), (got, want)
    one = trip[:1].contiguous()
    got = K.eval_ranks(desc, one, *K.filter_csr_build(known, one, int(z["E"]), int(z["R"]))).cpu().numpy()
    assert got.shape == (4, 1) and np.array_equal(got[:, 0], want[:, 0]), (got, want[:, 0])


# ---------------------------------------------------------------- edge shapes against the float64 restatement
def problem(seed, E, R, d1, d2, B, repeat=False, zipf=False, scale=3.0):
    rng = np.random.default_rng(seed)
    P = {TABLES[0]: rng.normal(size=(E, d1)) * scale / np.sqrt(d1), TABLES[1]: rng.normal(size=(R, d2)) * scale / np.sqrt(d2),
         TABLES[2]: rng.normal(size=(d2, d1 * d1)) * scale / np.sqrt(d1)}
    P = {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}
    h, t = rng.integers(E, size=B), rng.integers(E, size=B)
    r = np.minimum(rng.zipf(1.5, size=B) - 1, R - 1) if zipf else rng.integers(R, size=B)
    if repeat:
        h[B // 2:], r[B // 2:], t[B // 2:] = h[:B - B // 2], r[:B - B // 2], t[:B - B // 2]
    y1, y2 = (rng.random((B, E)) < 0.05).astype(np.float64), (rng.random((B, E)) < 0.05).astype(np.float64)
    y1[np.arange(B), t], y2[np.arange(B), h] = 1.0, 1.0
    return P, h, r, t, y1, y2


EDGES = {"odd": dict(E=70, R=5, d1=33, d2=7, B=5), "row_tile": dict(E=257, R=9, d1=64, d2=32, B=130),
         "repeated": dict(E=70, R=5, d1=33, d2=7, B=12, repeat=True), "zipf": dict(E=257, R=40, d1=48, d2=20, B=70, zipf=True)}


@pytest.mark.parametrize("dropouts", [(0.0, 0.0, 0.0), DROP], ids=["p0", "dropout"])
@pytest.mark.parametrize("case", sorted(EDGES))
def test_edge_shapes_match_float64(hip, case, dropouts):
    P, h, r, t, y1, y2 = problem(11, **EDGES[case])
    kw = dict(dropouts=dropouts, seed=(7 << 32) | 9, offset=5)
    ref, b = bounds(P, h, r, t, y1, y2, label_smoothing=0.1, **kw)
    check_step(case, fused(P, h, r, t, y1, y2, ls=0.1, **kw), ref, b)
    # the predictions under the same masks: the body op with the step's seed / offset on the rows [h; t], then the head
    from pykg2vec_amd import kernels as K
    m = model_for(P, dropouts)
    d = m.make_desc(train=True, seed=kw["seed"], offset=kw["offset"])
    x, _ = K.tucker_body_forward(d, hip.dev(np.concatenate([h, t])), hip.dev(np.concatenate([r, r])))
    p = K.head_1n_forward(x, m.ent_embeddings.weight.detach(), None).cpu().numpy()
    err = np.abs(p - np.concatenate([ref[2], ref[3]])).max()
    print(case, "preds err %.3g (bound %.3g)" % (err, b["preds"]))
    assert err <= b["preds"]


def test_core_gradient_is_bit_identical(hip):
    P, h, r, t, y1, y2 = problem(12, **EDGES["row_tile"])
    a = fused(P, h, r, t, y1, y2, DROP, seed=3, offset=1)[1]["W.weight"]
    b = fused(P, h, r, t, y1, y2, DROP, seed=3, offset=1)[1]["W.weight"]
    assert np.array_equal(a, b)
    c = fused(P, h, r, t, y1, y2, DROP, seed=4, offset=1)[1]["W.weight"]
    assert not np.array_equal(a, c)     # another seed: other masks
    p0 = [fused(P, h, r, t, y1, y2, seed=s)[1]["W.weight"] for s in (3, 4)]
    assert np.array_equal(p0[0], p0[1])   # p = 0 draws nothing: the seed cannot matter


def test_autograd_path_agrees_with_fused_step(hip):
    P, h, r, t, y1, y2 = problem(13, **EDGES["odd"])
    ref, b = bounds(P, h, r, t, y1, y2, label_smoothing=0.1)
    m = model_for(P)
    m.train()
    E = P[TABLES[0]].shape[0]
    loss = m.loss(m(hip.dev(t), hip.dev(r), direction="head"), m(hip.dev(h), hip.dev(r), direction="tail"),
                  torch.from_numpy(y2).float().cuda(), torch.from_numpy(y1).float().cuda(), 0.1, E)
    loss.backward()
    got = (loss.item(), {k: p.grad.cpu().numpy().astype(np.float64) for k, p in zip(TABLES, m.trainable_tensors())})
    check_step("autograd", got, ref, b)
    check_step("fused", fused(P, h, r, t, y1, y2, ls=0.1), ref, b)


# ---------------------------------------------------------------- production size, Trainer, Evaluator
def toy_config(hip, E, R, n, batch_size, seed=0, **kw):
    rng = np.random.default_rng(21)
    trip = np.unique(np.stack([rng.integers(E, size=2 * n), rng.integers(R, size=2 * n), rng.integers(E, size=2 * n)], 1), axis=0)
    trip = trip[rng.permutation(len(trip))][:n + 40]
    cfg = hip.make_config(E, R, {"neg_rate": 0}, trip[:n], trip[n:n + 20], trip[n + 20:], batch_size=batch_size, **kw)
    cfg.seed = seed
    return cfg


def test_production_size_step_with_adam(hip):
    from pykg2vec_amd.trainer import Trainer
    E, R, d, B = 14951, 1345, 200, 128
    P, h, r, t, y1, y2 = problem(14, E, R, d, d, B, scale=1.0)
    ref, b = bounds(P, h, r, t, y1, y2, dropouts=DROP, seed=5, offset=0, label_smoothing=0.1)
    cfg = toy_config(hip, E, R, 300, B, seed=5, optimizer="adam", lr=0.001, label_smoothing=0.1)
    tn = Trainer(model_for(P, DROP), cfg)
    tn.build_model()
    tn.model.train()
    loss = tn.train_step_projection(hip.dev(h), hip.dev(r), hip.dev(t), csr(y1), csr(y2)).item()
    got = (loss, {k: g.cpu().numpy().astype(np.float64) for k, g in zip(TABLES, tn.flat.grad_views)})
    check_step("production", got, ref, b)
    before = tn.flat.views[2].clone()
    tn._reduce_and_step()
    step = (tn.flat.views[2] - before).abs().max().item()
    assert 0.5e-3 < step < 1.5e-3, step     # Adam's first step moves a touched element by about lr


def test_trainer_end_to_end(hip):
    from pykg2vec_amd.trainer import Trainer
    from pykg2vec_amd import kernels as K

    def run():
        torch.manual_seed(0)
        from pykg2vec_amd.projection import TuckER
        m = TuckER(tot_entity=70, tot_relation=5, ent_hidden_size=20, rel_hidden_size=12, lmbda=0.0, input_dropout=0.3,
                   hidden_dropout1=0.4, hidden_dropout2=0.5)
        cfg = toy_config(hip, 70, 5, 300, 32, seed=9, optimizer="adam", lr=0.01, label_smoothing=0.1)
        tn = Trainer(m, cfg)
        tn.build_model()
        tn.generator = tn._new_generator()
        losses = [tn.train_model_epoch(e) for e in range(3)]
        return tn, cfg, losses

    tn, cfg, losses = run()
    print("epoch losses", losses)
    assert losses[2] < losses[0]
    tn2, _, losses2 = run()
    assert losses == losses2 and torch.equal(tn.model.W.weight, tn2.model.W.weight)    # the same seed: the same W bit for bit
    tn.model.eval()
    test = cfg.knowledge_graph.read_cache_data("triplets_test")
    ranks = tn.evaluator.rank_all(test, len(test)).cpu().numpy()
    known = np.concatenate([cfg.knowledge_graph.read_cache_data(k) for k in ("triplets_train", "triplets_valid", "triplets_test")])
    trip = hip.dev(test)
    csrs = K.filter_csr_build(hip.dev(known), trip, 70, 5)
    direct = K.tucker_eval_ranks(tn.model.make_desc(), trip, *csrs).cpu().numpy()
    assert np.array_equal(ranks, direct)
    with torch.no_grad():
        tn.evaluator.full_test(0)
    P = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in zip(TABLES, tn.model.trainable_tensors())}
    want, gap = tr.ranks(P, test, known)
    print("float64 rank gap", gap)
    if gap > 1e-5:
        assert np.array_equal(ranks, want)
