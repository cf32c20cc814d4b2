"""ProjE_pointwise on the HIP path (csrc/kge_proje.hip): parity with the reference's float64 outputs in tests/golden/ref_proje{,_neg}.npz
(exact ranks), the label-sparse loss kernel and the fused step at edge shapes against the float64 restatement of
tools/proje_reference.py with shared Philox masks, the clamps, the autograd path, the ordered row gradients and the public Trainer /
Evaluator classes.

Tolerances: on every test shape the plain fp32 numpy run of the same formulas (proje_reference with dtype=np.float32) is compared with
the float64 one; the HIP path is allowed FACTOR = 4 times that error per quantity (the loss, each gradient relative to its max-abs),
the factor covering another summation order in the dot products and in the atomics.  The errors are measured where they are used
(`bounds`), printed, and floored at one fp32 ulp of the quantity (2^-23 relative): a measured error of zero cannot be a bound.
DESIGN.md section 16 lists the figures of the fixture shape."""
import numpy as np
import pytest
import torch

from golden_util import skewed_triples
from test_proje_model import NAMES, SWITCHES, TABLES, fixture, pr, tables

pytestmark = pytest.mark.gpu
FACTOR = 4.0
ULP = 2.0 ** -23
ENT = TABLES[0]


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    """A Trainer reads the KGE_* A/B switches from the process environment, and other test modules of this suite leave some of them
    set: every test here starts without them."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def csr(y):
    """Positive CSR (off int64 [B + 1], ids int32 ascending) of the +1 entries of dense label rows."""
    off = np.concatenate([[0], np.cumsum((y > 0).sum(1))]).astype(np.int64)
    ids = np.concatenate([np.flatnonzero(row > 0) for row in y] + [np.zeros(0, np.int64)]).astype(np.int32)
    return torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda()


def dev_neg(neg):
    return None if neg is None else torch.from_numpy(np.asarray(neg, dtype=np.int32)).cuda()


def labels(y, neg):
    """The reference's label rows: the positives of y plus -1 on the negative ids that are no positive of the row."""
    out = (y > 0).astype(np.float64)
    if neg is not None:
        out[:, neg] -= (out[:, neg] == 0)
    return out


def model_for(P, p=0.0, lmbda=0.0, seed=0):
    from pykg2vec_amd.projection import ProjE_pointwise
    E, k = P[TABLES[0]].shape
    m = ProjE_pointwise(tot_entity=E, tot_relation=P[TABLES[1]].shape[0], hidden_size=k, lmbda=lmbda, hidden_dropout=p, seed=seed)
    m.load_state_dict({n: torch.from_numpy(np.asarray(P[n], dtype=np.float32)) for n in TABLES})
    return m.cuda()


def fused(P, h, r, t, y1, y2, neg, lmbda, p=0.0, seed=0, offset=0):
    """(loss, {table: gradient}) of kge_proje_train."""
    from pykg2vec_amd import kernels as K
    m = model_for(P, p, lmbda)
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=seed, offset=offset)
    loss = K.new_loss_buffer(ws[0].device)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()
    K.proje_train(d, dev(h), dev(r), dev(t), *csr(y1), *csr(y2), dev_neg(neg), lmbda, loss)
    return K.read_loss(loss).item(), {n: g.cpu().numpy().astype(np.float64) for n, g in zip(TABLES, gs)}


def bounds(P, h, r, t, y1, y2, neg, lmbda, **kw):
    """The float64 step and FACTOR x the fp32 restatement's error per quantity."""
    Y1, Y2 = labels(y1, neg), labels(y2, neg)
    with np.errstate(over="ignore"):
        ref = pr.step(P, h, r, t, Y1, Y2, lmbda, **kw)
        f32 = pr.step(P, h, r, t, Y1, Y2, lmbda, dtype=np.float32, **kw)
    b = {"loss": FACTOR * max(abs(f32["loss"] - ref["loss"]), ULP * abs(ref["loss"]))}
    for n in TABLES:
        b[n] = FACTOR * max(np.abs(f32["grads"][n] - ref["grads"][n]).max(), ULP * np.abs(ref["grads"][n]).max())
    return ref, b


def check_step(tag, got, ref, b):
    loss, g = got
    want, grads = (ref["loss"], ref["grads"]) if isinstance(ref, dict) else ref
    print(tag, "loss %.9g err %.3g (bound %.3g)" % (want, abs(loss - want), b["loss"]))
    bad = [] if abs(loss - want) <= b["loss"] else ["loss"]
    for n in TABLES:
        err = np.abs(g[n] - grads[n]).max()
        print(tag, n, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[n], np.abs(grads[n]).max()))
        if not err <= b[n]:
            bad.append(n)
    assert not bad, (tag, bad)


# ---------------------------------------------------------------- reference fixtures
@pytest.mark.parametrize("name", NAMES)
def test_fixture_parity(hip, name):
    from pykg2vec_amd import kernels as K
    z = fixture(name)
    P = tables(z)
    neg = z["neg"] if len(z["neg"]) else None
    lmbda = float(z["lmbda"])
    assert np.array_equal(labels(z["hr_t"], neg), z["hr_t"]) and np.array_equal(labels(z["tr_h"], neg), z["tr_h"])
    _, b = bounds(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], neg, lmbda)
    want = (float(z["loss"]), {n: z["grad." + n] for n in TABLES})
    check_step(name, fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], neg, lmbda), want, b)
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    trip = hip.dev(z["test"])
    t_off, t_ids, h_off, h_ids = K.filter_csr_build(hip.dev(known), trip, int(z["E"]), int(z["R"]))
    ties = torch.zeros((2, len(z["test"])), dtype=torch.int32, device="cuda")
    ranks = K.proje_eval_ranks(model_for(P).make_desc(), trip, t_off, t_ids, h_off, h_ids, ties=ties).cpu().numpy()
    assert np.array_equal(ranks, z["ranks"]), (ranks, z["ranks"])    # exact, all of them
    assert int(ties.sum()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_rank_pass_with_one_side_unfiltered_and_with_one_triple(hip, name):
    """The shared rank pass (csrc/kge_projection.hip) with an absent filter on either side and with n = 1: exact against the ranks
    the reference recorded."""
    from pykg2vec_amd import kernels as K
    z = fixture(name)
    desc = model_for(tables(z)).make_desc()
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


def test_evaluator_ranks_equal_the_restatement(hip):
    from pykg2vec_amd.evaluator import Evaluator
    z = fixture("proje_neg")
    P = tables(z)
    cfg = hip.make_config(70, 5, {"neg_rate": 1}, z["train"], z["valid"], z["test"], batch_size=9)
    m = model_for(P, p=0.5)     # the ranking calls draw no dropout
    ranks = Evaluator(m, cfg).rank_all(z["test"], len(z["test"])).cpu().numpy()
    want, gap = pr.ranks(P, z["test"], np.concatenate([z["train"], z["valid"], z["test"]]))
    assert gap > 1e-6 and np.array_equal(ranks, want) and np.array_equal(want, z["ranks"])
    with torch.no_grad():   # the reference Evaluator's hooks: topk(-prediction), i.e. candidate ids by ASCENDING prediction
        a, b, c = (hip.dev(z["test"][:1, i]) for i in range(3))
        tails = m.predict_tail_rank(a, b, topk=70).view(-1).cpu().numpy()
        heads = m.predict_head_rank(c, b, topk=70).view(-1).cpu().numpy()
    h, r, t = z["test"][0]
    # utils/evaluator.py:70-123 walks such a list from its END: the rank is the number of candidates behind the true one
    assert 69 - list(tails).index(t) == z["ranks"][1, 0] and 69 - list(heads).index(h) == z["ranks"][0, 0]
    assert sorted(tails) == sorted(heads) == list(range(70))
    assert m.dropout_offset == 0


# ---------------------------------------------------------------- edge shapes against the float64 restatement
def problem(seed, E, R, k, B, n_neg, duplicates=False, hub=False, covered=False, long_list=0, zipf=False, zeros=False, scale=3.0):
    """Tables on the fp32 grid, batch ids, dense positive rows of both directions and the batch's negative ids.  The logits stay within
    a few units (scale / sqrt(k) entity rows against tanh outputs)."""
    rng = np.random.default_rng(seed)
    P = {TABLES[0]: rng.normal(size=(E, k)) * scale / np.sqrt(k), TABLES[1]: rng.normal(size=(R, k))}
    for n in TABLES[2:]:
        P[n] = rng.normal(size=(1, k))
    if zeros:   # exact zeros: sign(0) = 0 in the regulariser's gradient
        P[TABLES[0]][rng.random((E, k)) < 0.2] = 0.0
        P[TABLES[1]][0] = 0.0
        P["De1.weight"][0, ::3] = 0.0
        P["Dr2.weight"][0, 1::2] = 0.0
    P = {n: v.astype(np.float32).astype(np.float64) for n, v in P.items()}
    if zipf:
        trip = skewed_triples(rng, B, E, R)
        h, r, t = trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()
    else:
        h, r, t = rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)
    if duplicates:   # the same (h, r) and (t, r) in several rows
        h[B // 2:], r[B // 2:], t[B // 2:] = h[:B - B // 2], r[:B - B // 2], t[:B - B // 2]
    y1, y2 = (rng.random((B, E)) < 0.03).astype(np.float64), (rng.random((B, E)) < 0.03).astype(np.float64)
    y1[np.arange(B), t], y2[np.arange(B), h] = 1.0, 1.0
    neg = rng.permutation(E)[:n_neg]
    if hub:          # one entity is a positive of every row, in both directions
        y1[:, 7], y2[:, 7] = 1.0, 1.0
    if covered:      # a row whose positives contain every negative id
        y1[1, neg], y2[B - 1, neg] = 1.0, 1.0
    if long_list:    # a row with `long_list` positives
        y1[2] = 0.0
        y1[2, rng.permutation(E)[:long_list]] = 1.0
        y2[0] = y1[2]
    return P, h, r, t, y1, y2, neg


EDGES = {"odd": dict(E=70, R=5, k=33, B=5, n_neg=70, covered=True),                 # the negatives are the whole table
         "tile": dict(E=257, R=9, k=64, B=130, n_neg=100, hub=True),
         "preset_width": dict(E=257, R=9, k=200, B=130, n_neg=100, duplicates=True, zeros=True),
         "wide": dict(E=70, R=5, k=257, B=5, n_neg=70, hub=True),
         "long_list": dict(E=331, R=5, k=33, B=5, n_neg=100, long_list=300),
         "zipf": dict(E=257, R=40, k=64, B=130, n_neg=100, zipf=True, duplicates=True)}


@pytest.mark.parametrize("negatives", [True, False], ids=["neg", "noneg"])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["p0", "dropout"])
@pytest.mark.parametrize("case", sorted(EDGES))
def test_fused_step_matches_float64(hip, case, p, negatives):
    P, h, r, t, y1, y2, neg = problem(31, **EDGES[case])
    if EDGES[case].get("long_list"):
        assert (y1 > 0).sum(1).max() == 300
    neg = neg if negatives else None
    kw = dict(p=p, seed=(7 << 32) | 9, offset=(1 << 33) + 5)
    ref, b = bounds(P, h, r, t, y1, y2, neg, 0.01, **kw)
    check_step(case, fused(P, h, r, t, y1, y2, neg, 0.01, **kw), ref, b)


@pytest.mark.parametrize("negatives", [True, False], ids=["neg", "noneg"])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["p0", "dropout"])
@pytest.mark.parametrize("case", sorted(EDGES))
def test_label_loss_matches_float64(hip, case, p, negatives):
    """kge_proje_label_loss alone, on the body's output of the case (x carries the dropout zeros), one row with NO positive."""
    from pykg2vec_amd import kernels as K
    P, h, r, t, y1, _, neg = problem(32, **EDGES[case])
    y1[len(h) - 1] = 0.0      # an empty positive list
    neg = neg if negatives else None
    E, k = P[ENT].shape
    x64, _ = pr.body(P, h, r, 0, pr.mask(0, len(h), k, p, seed=3, offset=1))
    x = x64.astype(np.float32)
    Y = labels(y1, neg)
    ref = pr.label_loss(x.astype(np.float64), P[ENT], Y)
    f32 = pr.label_loss(x, P[ENT], Y, dtype=np.float32)
    want = {"loss": ref[0], "dx": ref[1] @ P[ENT], "g_ent": ref[1].T @ x.astype(np.float64)}
    low = {"loss": f32[0], "dx": f32[1] @ P[ENT].astype(np.float32), "g_ent": f32[1].T @ x}
    ent = torch.from_numpy(P[ENT].astype(np.float32)).cuda()
    g_ent = torch.zeros_like(ent)
    loss = K.new_loss_buffer(ent.device)
    dx = K.proje_label_loss(torch.from_numpy(x).cuda(), ent, *csr(y1), dev_neg(neg), loss, g_ent)
    got = {"loss": K.read_loss(loss).item(), "dx": dx.cpu().numpy().astype(np.float64), "g_ent": g_ent.cpu().numpy().astype(np.float64)}
    bad = []
    for q in ("loss", "dx", "g_ent"):
        top = np.abs(want[q]).max()
        bound = FACTOR * max(np.abs(low[q] - want[q]).max(), ULP * top)
        err = np.abs(got[q] - want[q]).max()
        print(case, q, "err %.3g (bound %.3g, max-abs %.3g)" % (err, bound, top))
        if not err <= bound:
            bad.append(q)
    assert not bad, (case, bad)
    assert not dx[len(h) - 1].any() or negatives     # no label in the row: no gradient


def test_n_neg_zero_and_no_labels_at_all(hip):
    """An empty negative list is `no list`; a batch without a single label adds nothing and zeroes dx."""
    from pykg2vec_amd import kernels as K
    x = torch.randn(5, 33, device="cuda")
    ent = torch.randn(70, 33, device="cuda")
    off = torch.zeros(6, dtype=torch.int64, device="cuda")
    ids = torch.zeros(0, dtype=torch.int32, device="cuda")
    g_ent, loss = torch.zeros_like(ent), K.new_loss_buffer(ent.device)
    dx = K.proje_label_loss(x, ent, off, ids, torch.zeros(0, dtype=torch.int32, device="cuda"), loss, g_ent)
    assert K.read_loss(loss).item() == 0.0 and not dx.any() and not g_ent.any()


# ---------------------------------------------------------------- the clamps
LOG_CLAMP = -np.log(np.float64(np.float32(1e-10)))


def clamp_problem(E=70, R=5, k=33, B=12):
    """Column 0 decides every logit: ent[c][0] = w_c in +-{0.5, 2, 5, 45, 60}, the batch entities have |w| >= 5, De[0] = 1, Dr[0] =
    bc[0] = 0, so x[0] = tanh(w_e) = +-1 to 1e-4 and z = +-w_c up to the small other columns."""
    rng = np.random.default_rng(41)
    P = {TABLES[0]: rng.normal(size=(E, k)) * 0.05, TABLES[1]: rng.normal(size=(R, k)) * 0.05}
    for n in TABLES[2:]:
        P[n] = rng.normal(size=(1, k)) * 0.05
    w = rng.choice([0.5, 2.0, 5.0, 45.0, 60.0], size=E) * rng.choice([-1.0, 1.0], size=E)
    P[TABLES[0]][:, 0] = w
    for s in "12":
        P["De%s.weight" % s][0, 0], P["Dr%s.weight" % s][0, 0], P["bc%s.weight" % s][0, 0] = 1.0, 0.0, 0.0
    P = {n: v.astype(np.float32).astype(np.float64) for n, v in P.items()}
    big = np.flatnonzero(np.abs(w) >= 5.0)
    h, t, r = rng.choice(big, size=B), rng.choice(big, size=B), rng.integers(R, size=B)
    return P, h, r, t


def test_clamped_entries(hip):
    P, h, r, t = clamp_problem()
    E = P[ENT].shape[0]
    rng = np.random.default_rng(42)
    y1, y2 = (rng.random((len(h), E)) < 0.3).astype(np.float64), (rng.random((len(h), E)) < 0.3).astype(np.float64)
    neg = rng.permutation(E)
    ref, b = bounds(P, h, r, t, y1, y2, neg, 0.01)
    z = np.abs(np.concatenate([ref["logits_tail"], ref["logits_head"]]))
    Y = np.concatenate([labels(y1, neg), labels(y2, neg)])
    assert (z[Y != 0] > 40).sum() > 100 and not ((z > 14) & (z < 25)).any()    # on the float64 logits
    check_step("clamp", fused(P, h, r, t, y1, y2, neg, 0.01), ref, b)
    # only entries that a clamp catches (positives with z < -40, negatives with z > 40), row by row through the label kernel: each
    # contributes -log(1e-10) and no gradient at all
    from pykg2vec_amd import kernels as K
    ent = torch.from_numpy(P[ENT].astype(np.float32)).cuda()
    x = torch.from_numpy(pr.body(P, h, r, 0)[0].astype(np.float32)).cuda()
    count = 0
    for i in range(len(h)):
        zt = ref["logits_tail"][i]
        y, nneg = (zt < -40).astype(np.float64)[None], np.flatnonzero(zt > 40)
        g_ent, loss = torch.zeros_like(ent), K.new_loss_buffer(ent.device)
        dx = K.proje_label_loss(x[i:i + 1].contiguous(), ent, *csr(y), dev_neg(nneg), loss, g_ent)
        n = int(y.sum()) + len(nneg)
        count += n
        got = K.read_loss(loss).item()
        assert abs(got - n * LOG_CLAMP) <= 2 * ULP * n * LOG_CLAMP, (i, got, n * LOG_CLAMP)   # logf's and the total's rounding
        assert not dx.any() and not g_ent.any(), i      # no gradient passes a clamp
    assert count > 50


# ---------------------------------------------------------------- autograd path, reproducibility
def test_autograd_path_agrees_with_fused_step(hip):
    P, h, r, t, y1, y2, neg = problem(33, **EDGES["odd"])
    kw = dict(p=0.5, seed=11, offset=4)
    ref, b = bounds(P, h, r, t, y1, y2, neg, 0.01, **kw)
    m = model_for(P, p=0.5, lmbda=0.01, seed=11)
    m.eval()     # the reference draws this dropout under eval() too
    Y1, Y2 = (torch.from_numpy(labels(y, neg)).float().cuda() for y in (y1, y2))
    m.dropout_offset = 4
    tails = m(hip.dev(h), hip.dev(r), Y1, direction="tail")
    assert m.dropout_offset == 5     # one per call
    m.dropout_offset = 4             # the fused step draws both directions at one offset; the side separates them
    heads = m(hip.dev(t), hip.dev(r), Y2, direction="head")
    loss = m.loss(heads, tails) + m.get_reg(None, None, None)
    loss.backward()
    got = (loss.item(), {n: q.grad.cpu().numpy().astype(np.float64) for n, q in zip(TABLES, m.trainable_tensors())})
    check_step("autograd", got, ref, b)
    check_step("fused", fused(P, h, r, t, y1, y2, neg, 0.01, **kw), ref, b)


def test_row_gradients_are_bit_identical(hip):
    P, h, r, t, y1, y2, neg = problem(34, **EDGES["tile"])
    runs = [fused(P, h, r, t, y1, y2, neg, 0.01, p=0.5, seed=3, offset=1)[1] for _ in range(2)]
    for n in TABLES[2:]:
        assert np.array_equal(runs[0][n], runs[1][n]), n
        assert runs[0][n].any()
    other = fused(P, h, r, t, y1, y2, neg, 0.01, p=0.5, seed=4, offset=1)[1]
    assert not np.array_equal(runs[0]["De1.weight"], other["De1.weight"])     # another seed: other masks
    p0 = [fused(P, h, r, t, y1, y2, neg, 0.01, seed=s)[1]["De1.weight"] for s in (3, 4)]
    assert np.array_equal(p0[0], p0[1])   # p = 0 draws nothing: the seed cannot matter


# ---------------------------------------------------------------- Trainer
def test_three_adam_steps_through_the_trainer(hip):
    """Generator (negative lists from (seed, batch)) + Trainer (masks from (seed, step)) + Adam against the restatement driven with the
    same masks and lists, in float64 and, for the bound, in fp32."""
    import kge_oracle as ko
    from pykg2vec_amd.trainer import Trainer
    E, R, k, B, lr, lmbda, seed = 300, 7, 24, 16, 0.01, 0.01, 9
    rng = np.random.default_rng(51)
    trip = np.unique(np.stack([rng.integers(E, size=400), rng.integers(R, size=400), rng.integers(E, size=400)], 1), axis=0)
    trip = trip[rng.permutation(len(trip))][:3 * B + 40]
    train = trip[:3 * B]
    cfg = hip.make_config(E, R, {"neg_rate": 1}, train, trip[3 * B:3 * B + 20], trip[3 * B + 20:], optimizer="adam", lr=lr, batch_size=B)
    cfg.seed = seed
    P0 = problem(52, E, R, k, B, 100)[0]
    tn = Trainer(model_for(P0, p=0.5, lmbda=lmbda), cfg)
    tn.build_model()
    tn.generator = tn._new_generator()
    tn.generator.start_one_epoch(3)
    runs = {np.float64: {n: v.copy() for n, v in P0.items()}, np.float32: {n: v.astype(np.float32) for n, v in P0.items()}}
    state = {dt: ko.optimizer_init("adam", Q) for dt, Q in runs.items()}
    losses = {dt: [] for dt in runs}
    got = []
    for step in range(3):
        batch = next(tn.generator)
        h, r, t, (o1, i1), (o2, i2), neg = batch
        assert neg.numel() == 100
        got.append(tn.train_step_projection(*batch).item())
        tn._reduce_and_step()
        cpu = lambda x: x.cpu().numpy()
        Y1, Y2 = pr.dense_labels(cpu(o1), cpu(i1), E, cpu(neg)), pr.dense_labels(cpu(o2), cpu(i2), E, cpu(neg))
        for dt, Q in runs.items():
            out = pr.step(Q, cpu(h), cpu(r), cpu(t), Y1, Y2, lmbda, p=0.5, seed=seed, offset=step, dtype=dt)
            losses[dt].append(out["loss"])
            ko.optimizer_step("adam", Q, {n: out["grads"][n].astype(dt) for n in TABLES}, state[dt], lr)
    bad = []
    for step in range(3):
        want = losses[np.float64][step]
        bound = FACTOR * max(abs(losses[np.float32][step] - want), ULP * abs(want))
        print("step", step, "loss %.9g err %.3g (bound %.3g)" % (want, abs(got[step] - want), bound))
        if not abs(got[step] - want) <= bound:
            bad.append("loss %d" % step)
    for n, view in zip(TABLES, tn.flat.views):
        want = runs[np.float64][n]
        bound = FACTOR * max(np.abs(runs[np.float32][n] - want).max(), ULP * np.abs(want).max())
        err = np.abs(view.detach().cpu().numpy().reshape(want.shape) - want).max()
        print(n, "after 3 steps: err %.3g (bound %.3g, max-abs %.3g)" % (err, bound, np.abs(want).max()))
        if not err <= bound:
            bad.append(n)
    assert not bad, bad
    assert np.abs(runs[np.float64][ENT] - P0[ENT]).max() > 2.5 * lr      # three Adam steps moved the tables
