"""kge_silhouette (csrc/kge_silhouette.hip) against the numpy float64 restatement of its contract (tests/silhouette_ref.py).

Exact cases: rows are t_i v with integer t_i in [-100, 100] and an integer vector v of integer norm ((1) for dim 1; sixteen (3, 4)
pairs and a zero for dim 33, norm 20), so every |x|^2, dot product, distance (|t_i - t_j| |v|) and tile sum is an integer below 2^24:
exact in float32 in ANY order.  For cosine the rows are +- unit axes: distances 0, 1, 2.  s, a, b must equal the float64 restatement
rounded to float32 once; neighbor, count and the score outright (the float32 samples of these cases sum exactly in float64, so the
order of the score's sum does not show).  Every case runs under SIL_SPLIT = 1 and 3 and must leave identical bits.  Rows are strided
views whose padding holds NaN.

Band cases: normal rows against float64.  Every float32 distance is within rel = (dim + 4) 2^-24 max(|x_i|^2 + |x_j|^2) / min d^2 of
the true one (the expansion's worst case over the smallest squared distance), a tile sum adds 33 2^-24, and s = (b - a) / max(a, b)
moves by at most 4 (rel + 33 2^-24)."""
import numpy as np
import pytest
import torch

import tsne_ref
from silhouette_ref import silhouette_ref
from pykg2vec_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV, U = "cuda", 2.0 ** -24
NAMES = ("s", "a", "b", "neighbor", "count")


def dev_rows(a, pad=3):
    a = np.asarray(a, np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return buf[:, :a.shape[1]]


def run(X, label, k, metric="l2", split=None):
    K.set_switch("SIL_SPLIT", split)
    try:
        res = K.silhouette(dev_rows(X), torch.from_numpy(np.asarray(label, np.int32)).to(DEV), k, metric)
        return {name: getattr(res, name).cpu().numpy() for name in NAMES + ("score",)}
    finally:
        K.set_switch("SIL_SPLIT", None)


def sized(sizes, rng):
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes))


# name -> (labels, k, dim, rows with a NaN): tiles of 32 members, an empty cluster in the middle and at the end, one and many row tiles
def _cases():
    rng = np.random.default_rng(7)
    edges = np.concatenate([sized([1, 2, 31, 0, 32, 33, 64, 65, 0], rng), [-1, 4]])   # the last two rows get a NaN
    twins = np.array([0, 0, 1, 1, 2, 2])           # clusters 0 and 1 are four copies of one point: max(a, b) = 0, equal means
    return {"tile_edges": (edges, 9, 33, [228, 229]), "pair_apart": ([0, 1], 2, 1, []), "pair_together": ([0, 0], 2, 33, []),
            "k33_n33": (rng.integers(0, 33, 33), 33, 1, [5]), "k2_n129": (rng.integers(0, 2, 129), 2, 33, [0, 128]),
            "twins": (twins, 3, 33, [])}


CASES = _cases()
TWIN_T = np.array([5, 5, 5, 5, 10, 20])


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_rows_match_the_reference_outright_under_every_split(name, metric):
    label, k, dim, nan_rows = CASES[name]
    label = np.asarray(label)
    n, rng = len(label), np.random.default_rng(len(name))
    if metric == "cosine":
        X = np.zeros((n, dim), np.float32)
        X[np.arange(n), rng.integers(0, min(dim, 3), n)] = rng.choice([-1.0, 1.0], n)
        if name == "twins":
            X[:] = 0
            X[np.arange(6), [0, 0, 0, 0, 1, 2]] = 1.0
    else:
        v = np.ones(1) if dim == 1 else np.array([3, 4] * 16 + [0])
        t = TWIN_T if name == "twins" else rng.integers(-100, 101, n)
        X = (t[:, None] * v[None, :]).astype(np.float32)
    X[nan_rows, dim // 2] = np.nan
    want = dict(zip(NAMES + ("score",), silhouette_ref(X, label, k, metric)))
    got1, got3 = run(X, label, k, metric, split=1), run(X, label, k, metric, split=3)
    for key in NAMES + ("score",):
        assert np.array_equal(got1[key], np.atleast_1d(want[key]).astype(got1[key].dtype), equal_nan=True), key
        assert got1[key].tobytes() == got3[key].tobytes(), key
    if name == "twins":
        assert got1["neighbor"].tolist() == [1, 1, 0, 0, 0, 0] and got1["s"][:4].tolist() == [0] * 4 and got1["b"][0] == 0


@pytest.mark.parametrize("n, k, dim", [(257, 5, 100), (1025, 37, 33)])
def test_normal_rows_stay_inside_the_propagated_band_and_repeat(n, k, dim):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    C = rng.standard_normal((k, dim))
    label = np.argmin(((X[:, None, :] - C[None]) ** 2).sum(2), 1)
    s, a, b, neighbor, count, score, D = silhouette_ref(X, label, k)
    d2, sq = D[~np.eye(n, dtype=bool)] ** 2, (X.astype(np.float64) ** 2).sum(1)
    assert d2.min() > 0                                             # no two rows coincide: the bound is finite
    tol = 4 * ((dim + 4) * U * np.sort(sq)[-2:].sum() / d2.min() + 33 * U)
    got, again = run(X, label, k), run(X, label, k)
    print("band", n, k, dim, "tol", tol, "worst", np.abs(got["s"] - s).max(), "score", got["score"][0], score)
    assert np.abs(got["s"] - s).max() <= tol and abs(got["score"][0] - score) <= tol and np.array_equal(got["count"], count)
    assert all(got[key].tobytes() == again[key].tobytes() for key in got)


def test_evaluator_scores_the_blobs_and_chooses_their_number():
    from pykg2vec_amd.evaluator import Evaluator
    from test_hip_tsne import _model
    X, blob = tsne_ref.clustered(300, 50, clusters=6, seed=5, centre_scale=3.0)
    m, cfg = _model("transe", 300, 11, 50, dict(ent_embeddings=X))
    ev = Evaluator(m, cfg)
    s, _, _, neighbor, count, score, D = silhouette_ref(X, blob, 6)
    sq = (X.astype(np.float64) ** 2).sum(1)
    tol = 4 * (54 * U * np.sort(sq)[-2:].sum() / (D[~np.eye(300, dtype=bool)] ** 2).min() + 33 * U)
    got_score, samples = ev.silhouette_vectors(torch.from_numpy(X), blob)
    direct = K.silhouette(torch.from_numpy(X).to(DEV), torch.from_numpy(blob.astype(np.int32)).to(DEV), 6)
    assert abs(got_score - score) <= tol and np.abs(samples.cpu().numpy() - s).max() <= tol
    assert torch.equal(samples, direct.s) and got_score == direct.score.item() and ev.silhouette_entities(blob)[0] == got_score
    assert ev.last_silhouette["counts"].tolist() == count.tolist() and int(ev.last_silhouette["invalid_rows"]) == 0
    assert np.array_equal(ev.last_silhouette["neighbor"].cpu().numpy(), neighbor)
    best, scores = ev.choose_n_clusters([2, 3, 6, 9])
    assert best == 6 and sorted(scores) == [2, 3, 6, 9] and abs(scores[6] - score) <= tol
