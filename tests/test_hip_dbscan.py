"""kge_dbscan (csrc/kge_dbscan.hip) against the numpy float64 restatement of its contract (tests/dbscan_ref.py): every output is an
integer and a unique function of the eps-graph, so everything is compared outright, under DBS_SPLIT = 1 and 3, on strided rows whose
padding holds NaN.  Exact cases: rows t_i v with integer t_i and v, or integer grid points, and an integer eps: every |x|^2, dot
product and squared distance is an integer below 2^24, so the float32 test equals the float64 one in ANY order; for cosine +- unit
axes (distances 0, 1, 2) and eps 0 or 1.  Band cases: normal rows; a float32 squared distance is within rel eps^2 of the true one,
rel = (dim + 4) 2^-24 max_ij(|x_i|^2 + |x_j|^2) / eps^2, and the test first asserts on the CPU that no float64 squared distance lies
inside eps^2 (1 +- rel): a condition on the inputs, not a tolerance."""
import numpy as np
import pytest
import torch

import tsne_ref
from dbscan_ref import dbscan_ref
from test_hip_silhouette import dev_rows   # strided device rows whose padding holds NaN
from pykg2vec_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV, U = "cuda", 2.0 ** -24
NAMES = ("label", "core", "count", "n_clusters")
# dim -> (v, the range of t, eps): eps^2 = 3600 admits |t_i - t_j| |v| <= 60
LINES = {1: (np.ones(1), 1500, 60.0), 33: (np.array([3, 4] * 16 + [0]), 100, 60.0), 65: (np.array([3, 4] * 32 + [0]), 50, 60.0)}


def run(X, eps, min_samples, metric="l2", split=None):
    K.set_switch("DBS_SPLIT", split)
    try:
        res = K.dbscan(dev_rows(X), eps, min_samples, metric)
        return {name: getattr(res, name).cpu().numpy() for name in NAMES + ("rounds",)}
    finally:
        K.set_switch("DBS_SPLIT", None)


def check(X, eps, min_samples, metric="l2"):
    want = dict(zip(NAMES, dbscan_ref(X, eps, min_samples, metric)))
    got = None
    for split in (1, 3):
        got = run(X, eps, min_samples, metric, split)
        for key in NAMES:
            assert np.array_equal(got[key], np.atleast_1d(want[key]).astype(got[key].dtype)), (key, split, min_samples, eps)
        assert 1 <= got["rounds"][0] <= max(1, int(want["core"].sum()))   # the bound of DESIGN section 37
    return got


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("dim", [1, 33, 65])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65, 129])
def test_exact_rows_match_the_reference_outright_under_every_split(n, dim, metric):
    rng = np.random.default_rng(1000 * n + dim)
    if metric == "cosine":
        X = np.zeros((n, dim), np.float32)
        X[np.arange(n), rng.integers(0, min(dim, 3), n)] = rng.choice([-1.0, 1.0], n)
        radii = (0.0, 1.0)
    else:
        v, span, eps = LINES[dim]
        X = (rng.integers(-span, span + 1, n)[:, None] * v[None, :]).astype(np.float32)
        radii = (eps, 0.0)
    nan_rows = [n // 2, n - 1] if n >= 3 else []
    X[nan_rows, dim // 2] = np.nan
    for eps in radii:
        for min_samples in (1, 2, n, n + 1):   # every valid row a core ... no core at all
            got = check(X, eps, min_samples, metric)
            assert (got["label"][nan_rows] == -1).all() and not got["count"][nan_rows].any() and not got["core"][nan_rows].any()
            assert min_samples <= n or (got["n_clusters"][0] == 0 and (got["label"] == -1).all())


def _grids():
    rng = np.random.default_rng(3)
    path = np.stack([np.arange(70), np.zeros(70)], 1)
    block = lambda x0: [(x0 + x, y) for x in range(3) for y in range(2)]   # six points, each with five of them within 2
    # row 0 borders only the second block: cluster 1 although its id is the lowest; (4, 0) is within 2 of a core of either block: the
    # lower number; (4, 2) is within 2 of (4, 0) only, which is no core: noise
    borders = np.array([(10, 0)] + block(0) + [(4, 0), (4, 2)] + block(6))
    twins = np.array([(1, 2)] * 3 + [(3, 4)] * 2 + [(5, 6)])
    return {"path_permuted": (path[rng.permutation(70)], 1.0, 2, [0] * 70), "path_descending": (path[::-1], 1.0, 2, [0] * 70),
            "borders": (borders, 2.0, 5, [1] + [0] * 6 + [0, -1] + [1] * 6), "duplicates": (twins, 0.0, 2, [0, 0, 0, 1, 1, -1])}


GRIDS = _grids()


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grid_shapes_paths_borders_numbering_and_duplicates(name):
    X, eps, min_samples, labels = GRIDS[name]
    got = check(X, eps, min_samples)
    print(name, "rounds", got["rounds"][0])
    assert got["label"].tolist() == labels


@pytest.fixture(scope="module", params=[33, 100])
def band(request):
    dim = request.param
    X, _ = tsne_ref.clustered(129, dim, clusters=4, seed=dim, centre_scale=1.5)
    D = dbscan_ref(X, 1.0, 5)[4]
    eps = float(np.float32(1.01 * np.sqrt(np.median(np.sort(D, 1)[:, 4]))))   # just past the median distance to the fourth nearest
    sq = (X.astype(np.float64) ** 2).sum(1)
    rel = (dim + 4) * U * np.sort(sq)[-2:].sum() / eps ** 2
    off = np.abs(D[~np.eye(129, dtype=bool)] / eps ** 2 - 1.0)
    print("band", dim, "eps", eps, "rel", rel, "nearest", off.min())
    assert off.min() > rel        # a condition on the inputs: no pair is near enough to eps for float32 to decide otherwise
    return X, eps


def test_normal_rows_match_outside_the_band_and_reversed_rows_give_the_same_components(band):
    X, eps = band
    a, b = check(X, eps, 5), run(X[::-1].copy(), eps, 5)
    assert a["n_clusters"][0] >= 1 and (a["label"] == -1).any() and (a["core"] == 0).any()
    la, lb, core = a["label"], b["label"][::-1], a["core"] == 1
    assert np.array_equal(a["count"], b["count"][::-1]) and np.array_equal(a["core"], b["core"][::-1])   # a symmetric pair test
    assert np.array_equal(la == -1, lb == -1) and a["n_clusters"][0] == b["n_clusters"][0]
    pairs = set(zip(la[core].tolist(), lb[core].tolist()))                       # cores: the same partition, renumbered
    assert len(pairs) == a["n_clusters"][0] == len({p for p, _ in pairs}) == len({q for _, q in pairs})


def test_evaluator_labels_feed_the_silhouette_and_suggest_eps_reads_the_k_distances():
    from pykg2vec_amd.evaluator import Evaluator
    from test_hip_tsne import _model
    X, _ = tsne_ref.clustered(300, 50, clusters=6, seed=5, centre_scale=3.0)
    m, cfg = _model("transe", 300, 11, 50, dict(ent_embeddings=X))
    ev = Evaluator(m, cfg)
    kth = np.sqrt(np.sort(dbscan_ref(X, 1.0, 5)[4], 1)[:, 4])
    eps = ev.suggest_eps(5)
    assert abs(eps - np.quantile(kth, 0.9)) <= 1e-4 * eps
    labels = ev.dbscan_vectors(torch.from_numpy(X), eps)
    direct = K.dbscan(torch.from_numpy(X).to(DEV), eps, 5)
    assert torch.equal(labels, direct.label.long()) and torch.equal(ev.dbscan_entities(eps), labels)
    info = ev.last_dbscan
    noise = int(info["noise_rows"])
    assert info["n_clusters"] == 6 and 0 < noise < 150 and noise == int((labels < 0).sum()) and info["rounds"] >= 1
    assert torch.equal(info["core"], direct.core.bool()) and torch.equal(info["neighbor_counts"], direct.count)
    score, _ = ev.silhouette_vectors(torch.from_numpy(X), labels)
    assert int(ev.last_silhouette["invalid_rows"]) == noise and score > 0.3
