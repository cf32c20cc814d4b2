"""kge_knn_rows (csrc/kge_knn.hip) against the numpy restatement of its contract (tests/knn_ref.py).

Exact cases: table and query entries are integers in [-8, 8], so with dim <= 2048 every product, every partial sum and
|q|^2 + |c|^2 - 2 q.c is an integer below 2^24 -- exact in float32 in ANY summation order.  Ids, counts and score bits must equal
the reference outright; L2 is compared with np.sqrt of the float32 integer (sqrt is correctly rounded on both sides, and distinct
squared distances below 2^22 keep distinct float32 roots, so the order by distance is the order by squared distance).

Band cases: normal-random rows against float64.  tol is DERIVED.  With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy
and Stability of Numerical Algorithms, 3.1-3.4), a length-dim fmaf chain in any order satisfies
    |fl(q.c) - q.c| <= gamma_dim * A,   A = sum |q_i| |c_i|,
which is the dot metric's tol.  Carried through the other formulas:
  cosine  fl(dot) / fl(|q| |c|): each norm is the root of a positive sum of dim fmaf terms (relative error gamma_dim / 2 + u after the
          root), their product and the division add u each, so the denominator is off by at most rho = gamma_(dim + 5) relatively and
          tol = gamma_dim * A / (|q| |c|) * (1 + 2 rho) + 2 rho * |cos|;
  l2      returned distances are recomputed directly: d_i = fl(q_i - c_i) carries u, d_i^2 two of them, the positive sum gamma_dim,
          the root halves the relative error and adds u: tol = dist * (gamma_(dim + 2) / 2 + 2 u).  WHICH rows are returned is decided
          by the expansion fl(fl(|q|^2 + |c|^2) - 2 fl(q.c)) clamped at 0, whose three terms add (each norm gamma_dim of itself, the
          product term 2 gamma_dim A, the two roundings u of their results): in squared distance
          tol2 = gamma_(dim + 2) * (|q|^2 + |c|^2 + 2 A).
The selection property is checked over ALL left-out candidates, not only the best one: returned r and left-out o satisfy
s_r >= s_o - tol_r - tol_o (dot, cosine) and d_r^2 <= d_o^2 + tol2_r + tol2_o (l2), since the kernel saw r ahead of o.  No case is
left out."""
import numpy as np
import pytest
import torch

import hip_util
import knn_ref
import topk_ref
from golden_util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_ROWS = [1, 31, 32, 33, 63, 65, 257, 1025]
KS = [1, 5, 32, 127, 128]
DIMS = [1, 2, 3, 5, 31, 33, 100, 515]
NQS = [1, 31, 33, 130]
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def dev_rows(a, pad=0, fill=0.0):
    """float32 device tensor of the rows of `a`; pad > 0: a strided view of a wider buffer whose padding holds `fill`."""
    a = np.asarray(a, np.float32)
    if not pad:
        return torch.from_numpy(a).to(DEV)
    buf = torch.full((a.shape[0], a.shape[1] + pad), float(fill), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return buf[:, :a.shape[1]]


def run(table, queries, k, metric, self_ids=None, pad=0, fill=0.0):
    from pykg2vec_amd import kernels as K
    s = None if self_ids is None else torch.as_tensor(np.asarray(self_ids), dtype=torch.int64, device=DEV)
    out = K.knn_rows(dev_rows(table, pad, fill), dev_rows(queries, pad, fill), k, metric=metric, self_ids=s)
    return tuple(x.cpu().numpy() for x in out)


def exact_scores(table, queries, metric):
    """The float32 scores an exact kernel returns on integer rows: dot as it is, l2 the float32 root of the integer."""
    t, q = np.asarray(table, np.int64), np.asarray(queries, np.int64)
    if metric == "dot":
        return (q @ t.T).astype(np.float32)
    d2 = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)
    assert d2.max(initial=0) < 2 ** 22
    return np.sqrt(d2.astype(np.float32))


def assert_exact(got, table, queries, k, metric, self_ids=None):
    want = knn_ref.knn_ref(table, queries, k, metric, self_ids, scores=exact_scores(table, queries, metric))
    topk_ref.assert_same(got, want)


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


# (n_rows, k) in full; dim, nq, the self-id mode and the stride cycle through their values, every value at least once
EXACT = [(n, k, DIMS[(i * len(KS) + j) % len(DIMS)], NQS[(i + j) % len(NQS)], (i + 2 * j) % 3, (i + j) % 2)
         for i, n in enumerate(N_ROWS) for j, k in enumerate(KS)]
assert {c[2] for c in EXACT} == set(DIMS) and {c[3] for c in EXACT} == set(NQS)


@pytest.mark.parametrize("n_rows, k, dim, nq, self_mode, strided", EXACT)
def test_exact_integer_rows_match_the_reference_outright(n_rows, k, dim, nq, self_mode, strided):
    rng = np.random.default_rng(1000 * n_rows + 10 * k + dim)
    table, queries = ints(rng, (n_rows, dim)), ints(rng, (nq, dim))
    self_ids = None
    if self_mode:
        self_ids = rng.integers(n_rows, size=nq)
        if self_mode == 2:
            self_ids[::2] = -1
    for metric in ("dot", "l2"):
        # strided rows whose padding would win (dot) or lose the true neighbours (l2) if it were read
        got = run(table, queries, k, metric, self_ids, pad=3 if strided else 0, fill=100.0)
        assert_exact(got, table, queries, k, metric, self_ids)
        live = n_rows - (np.zeros(nq, np.int64) if self_ids is None else (self_ids >= 0))
        assert np.array_equal(got[2], np.minimum(k, live))


@pytest.mark.parametrize("k", [1, 128])
@pytest.mark.parametrize("direction", ["improving", "worsening"])
def test_order_stress_scores_monotone_in_the_id(k, direction):
    """Candidates whose score improves strictly with the id turn every step's winners over (a compaction per step); the reverse
    order appends nothing after the first k."""
    n = 1025
    ids = np.arange(n, dtype=np.float32)
    table = np.stack([ids, np.ones(n, np.float32)], 1)
    sign = 1.0 if direction == "improving" else -1.0
    queries = np.stack([sign * np.arange(1, 34, dtype=np.float32), np.zeros(33, np.float32)], 1)       # dot = +- m * id
    assert_exact(run(table, queries, k, "dot"), table, queries, k, "dot")
    far = np.stack([np.full(33, 1100.0 if direction == "improving" else -75.0, np.float32), np.arange(33, dtype=np.float32)], 1)
    assert_exact(run(table, far, k, "l2"), table, far, k, "l2")                                       # distance falls / grows with id


@pytest.mark.parametrize("metric", knn_ref.METRICS)
def test_constant_table_is_one_tie_group_in_id_order(metric):
    n, k = 1025, 128
    table = np.tile(np.asarray([[3.0, -4.0, 0.0]], np.float32), (n, 1))
    queries = np.asarray([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0], [3.0, -4.0, 0.0]], np.float32)
    self_ids = np.asarray([5, -1, 0])
    ids, vals, count = run(table, queries, k, metric, self_ids)
    assert np.array_equal(count, [k] * 3)
    assert np.array_equal(ids[0], [i for i in range(k + 1) if i != 5]) and np.array_equal(ids[1], np.arange(k))
    assert np.array_equal(ids[2], np.arange(1, k + 1))
    want = {"dot": [-5.0, 0.0, 25.0], "cosine": [-5.0 / 15.0, 0.0, 1.0], "l2": [np.sqrt(np.float32(44.0)), 5.0, 0.0]}[metric]
    assert (vals == vals[:, :1]).all()
    assert np.allclose(vals[:, 0], want, rtol=4 * U, atol=0) and vals[1, 0] == want[1]      # the zero query: cosine 0 to everything


def test_planted_duplicates_are_at_distance_zero_and_first():
    rng = np.random.default_rng(7)
    n, dim = 257, 33
    table = rng.normal(size=(n, dim)).astype(np.float32)            # not integers: the direct recomputation makes the zero exact
    a, b = 40, 201
    table[b] = table[a]
    ids, vals, _ = run(table, table, 5, "l2", np.arange(n))
    assert ids[a, 0] == b and ids[b, 0] == a
    assert vals[a, 0].view(np.uint32) == 0 and vals[b, 0].view(np.uint32) == 0      # bit for bit +0.0
    ids, vals, _ = run(table, table[[a, b]], 5, "l2")
    assert ids[:, :2].tolist() == [[a, b], [a, b]] and (vals[:, :2].view(np.uint32) == 0).all()     # self_ids absent: a before b


@pytest.mark.parametrize("metric", knn_ref.METRICS)
def test_nan_rows_and_queries_come_last_in_id_order(metric):
    rng = np.random.default_rng(11)
    n, dim = 65, 5
    table, queries = ints(rng, (n, dim)), ints(rng, (4, dim))
    table[17, 3] = np.nan
    queries[2, 0] = np.nan
    ids, vals, count = run(table, queries, n, metric)
    assert np.array_equal(count, [n] * 4)
    for q in (0, 1, 3):
        assert ids[q, -1] == 17 and np.isnan(vals[q, -1]) and not np.isnan(vals[q, :-1]).any()
        assert sorted(ids[q].tolist()) == list(range(n))
    assert np.array_equal(ids[2], np.arange(n)) and np.isnan(vals[2]).all()         # a NaN query: every score NaN, id order
    if metric != "cosine":
        want = knn_ref.knn_ref(table, queries, n, metric, scores=np.where(np.isnan(knn_ref.scores64(table, queries, metric)), np.nan,
                                                                           exact_scores(np.nan_to_num(table), np.nan_to_num(queries), metric)))
        assert np.array_equal(ids, want[0]) and np.array_equal(vals, want[1], equal_nan=True)


@pytest.mark.parametrize("k", [5, 128])
def test_split_independence(k, monkeypatch):
    rng = np.random.default_rng(3)
    table = np.round(rng.normal(size=(1025, 31)) * 4).astype(np.float32) / 4          # ties included
    queries = table[rng.integers(1025, size=33)] + np.round(rng.normal(size=(33, 31))).astype(np.float32)
    self_ids = rng.integers(1025, size=33)
    for metric in knn_ref.METRICS:
        monkeypatch.delenv("KGE_KNN_SPLIT", raising=False)
        base = run(table, queries, k, metric, self_ids)
        for split in ("1", "2", "7"):
            monkeypatch.setenv("KGE_KNN_SPLIT", split)
            got = run(table, queries, k, metric, self_ids)
            for x, y in zip(got, base):
                assert x.tobytes() == y.tobytes(), (metric, split)


@pytest.fixture(scope="module")
def band_data():
    out = {}
    for dim in (100, 400):
        rng = np.random.default_rng(dim)
        out[dim] = rng.normal(size=(4097, dim)).astype(np.float32), rng.normal(size=(70, dim)).astype(np.float32)
    return out


@pytest.mark.parametrize("metric", knn_ref.METRICS)
@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("dim", [100, 400])
def test_band_against_float64(band_data, dim, k, metric):
    """See the module docstring for the derivation of tol."""
    table, queries = band_data[dim]
    ids, vals, count = run(table, queries, k, metric)
    assert np.array_equal(count, [k] * len(queries)) and (ids >= 0).all()
    t, q = table.astype(np.float64), queries.astype(np.float64)
    S = knn_ref.scores64(table, queries, metric)
    A = np.abs(q) @ np.abs(t).T
    qn2, tn2 = (q * q).sum(1)[:, None], (t * t).sum(1)[None, :]
    rho = gamma(dim + 5)
    if metric == "dot":
        tol, sel, sel_tol = gamma(dim) * A, -S, gamma(dim) * A
    elif metric == "cosine":
        tol = gamma(dim) * A / np.sqrt(qn2 * tn2) * (1 + 2 * rho) + 2 * rho * np.abs(S)
        sel, sel_tol = -S, tol
    else:
        tol = S * (gamma(dim + 2) / 2 + 2 * U)
        sel, sel_tol = S * S, gamma(dim + 2) * (qn2 + tn2 + 2 * A)
    rows = np.arange(len(queries))[:, None]
    err = np.abs(vals.astype(np.float64) - S[rows, ids])
    print(metric, dim, k, "max err / tol", (err / tol[rows, ids]).max())
    assert (err <= tol[rows, ids]).all()
    # selection: no returned candidate is behind a left-out one by more than the two pairs' tol (sel: lower is nearer)
    inside = np.zeros(S.shape, dtype=bool)
    inside[rows, ids] = True
    assert (inside.sum(1) == k).all()                                  # k distinct ids per row
    worst_in = np.where(inside, sel - sel_tol, -np.inf).max(1)
    best_out = np.where(inside, np.inf, sel + sel_tol).min(1)
    assert (worst_in <= best_out).all()
    # order of the returned list: (returned bits, id)
    better = vals[:, :-1] < vals[:, 1:] if metric == "l2" else vals[:, :-1] > vals[:, 1:]
    assert (better | ((vals[:, :-1] == vals[:, 1:]) & (ids[:, :-1] < ids[:, 1:]))).all()


# ------------------------------------------------------------------------------------------------------------------- end to end
def _evaluator(case):
    from pykg2vec_amd.evaluator import Evaluator
    c = Case(case)
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    m = hip_util.model_from_case(c)
    for p in m.parameter_list:        # integer rows: the search is exact and the reference's order is the kernel's
        p.weight.data.copy_(torch.round(p.weight.data * 8 / p.weight.data.abs().max()))
    return c, m, Evaluator(m, cfg)


@pytest.mark.parametrize("case", ["transe_l2", "complex"])
def test_nearest_entities_end_to_end(case):
    c, m, ev = _evaluator(case)
    W = np.concatenate([p.weight.detach().cpu().numpy() for p in m.parameter_list if p.weight.shape[0] == c.E and
                        p.name.startswith(("ent_", "emb_e_"))], 1)
    assert W.shape[1] == (2 if case == "complex" else 1) * m.parameter_list[0].weight.shape[1]
    ids = np.random.default_rng(0).integers(c.E, size=40)
    k = min(10, c.E - 1)
    for metric in ("dot", "l2"):
        got, vals = ev.nearest_entities(ids, topk=k, metric=metric)
        want = knn_ref.knn_ref(W, W[ids], k, metric, ids, scores=exact_scores(W, W[ids], metric))
        assert np.array_equal(got.cpu().numpy(), want[0]) and np.array_equal(vals.cpu().numpy(), want[1])
    assert not (got.cpu().numpy() == ids[:, None]).any()
    got, _ = ev.nearest_entities(ids, topk=1, metric="l2", exclude_self=False)
    d0 = exact_scores(W, W[ids], "l2")
    assert np.array_equal(got.cpu().numpy()[:, 0], np.argmin(d0, 1))       # the row itself, or a lower-id copy of it


def test_translated_vectors_find_what_predict_tails_finds():
    """TransE scores || h^ + r^ - t^ || over NORMALISED rows, so the tables are given unit rows first: then ent[h] + rel[r] against the
    entity matrix under "l2" is the tail sweep's energy, up to float32 rounding of either path (some 1e-7 at these sizes; the
    float64 distances of neighbouring places differ by more than 1e-5, checked here, so the two orders agree)."""
    from pykg2vec_amd.evaluator import Evaluator
    c = Case("transe_l2")
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    m = hip_util.model_from_case(c)
    for p in m.parameter_list:
        p.weight.data.copy_(torch.nn.functional.normalize(p.weight.data.double(), dim=1).float())
    ev = Evaluator(m, cfg)
    rng = np.random.default_rng(1)
    h, r = rng.integers(c.E, size=30), rng.integers(c.R, size=30)
    ent, rel = m.ent_embeddings.weight.detach(), m.rel_embeddings.weight.detach()
    k = min(10, c.E - 1)
    v = ent[torch.as_tensor(h, device=DEV)] + rel[torch.as_tensor(r, device=DEV)]
    d = np.sort(knn_ref.scores64(ent.cpu().numpy(), v.cpu().numpy(), "l2"), 1)[:, :k + 1]
    assert np.diff(d, axis=1).min() > 1e-5
    got, _ = ev.nearest_to_vectors(v, kind="entity", topk=k, metric="l2")
    want, _ = ev.predict_tails(h, r, topk=k)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_find_duplicates_end_to_end():
    c, m, ev = _evaluator("transe_l2")
    w = m.ent_embeddings.weight.data
    w[7] = w[2]
    w[11] = w[2]
    pairs, scores = ev.find_duplicates(kind="entity", metric="l2", threshold=0.0, topk=4)
    W = w.cpu().numpy()
    d0 = exact_scores(W, W, "l2")
    a, b = np.nonzero(np.triu(d0 == 0, 1))
    assert {(2, 7), (2, 11), (7, 11)} <= set(zip(a.tolist(), b.tolist()))
    if (np.triu(d0 == 0, 1).sum(1) < 4).all():         # every copy fits the topk neighbours: the list is complete
        assert pairs.cpu().tolist() == [list(p) for p in zip(a.tolist(), b.tolist())]
    assert (scores == 0).all() and pairs.dtype == torch.int64
