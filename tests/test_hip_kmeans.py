"""kge_kmeans_* (csrc/kge_kmeans.hip) against the numpy restatement of its contract (tests/kmeans_ref.py).

Exact cases: row and centroid entries are integers in [-8, 8], so with dim <= 2048 every product, norm, key, squared distance and chunk
sum is an integer below 2^24 -- exact in float32 in ANY order: labels, dist2, counts, seeded ids and the centroids after one update
(float32(float64 sum / count) on both sides) must equal the restatement outright.  Rows are strided views whose padding holds NaN: a
read past dim shows.

Band cases: normal-random rows against float64, u = 2^-24, gamma_n = n u / (1 - n u).  The chosen centroid r and every other o satisfy
d2_r <= d2_o + tol2_r + tol2_o with tol2 = gamma_(dim+2) (|x|^2 + |c|^2 + 2 sum |x_j||c_j|), the bound derived in test_hip_knn.py's
header for the same expansion (the row's own |x|^2 is common to all keys); dist2 is recomputed directly: gamma_(dim+2)-relative; a
centroid column is a float32 chunk sum (gamma_CHUNK of sum |x|) added, divided and rounded once (u |c|):
gamma_(CHUNK+1) sum_members |x_ic| / count + u |c|."""
import numpy as np
import pytest
import torch

import kmeans_ref
import tsne_ref
from kmeans_ref import CHUNK
from pykg2vec_amd import kernels as K

pytestmark = pytest.mark.gpu

DEV, U = "cuda", 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def dev_rows(a, pad=3):
    """float32 device rows of `a` as a strided view of a wider buffer whose padding holds NaN."""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return buf[:, :a.shape[1]]


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


# n: the row tiles (32; 64 from 32768 rows on), k: 32 centroids per wave, 128 per step, dim: the 32-column slabs; k == n twice
EXACT = [(1, 1, 1), (31, 2, 3), (33, 31, 31), (63, 33, 33), (65, 1, 100), (257, 127, 515), (1025, 129, 1), (1025, 300, 3), (257, 129, 31),
         (65, 2, 33), (1025, 127, 100), (63, 31, 515), (33, 33, 3), (31, 31, 100), (32801, 129, 33)]


@pytest.mark.parametrize("n, k, dim", EXACT)
def test_exact_integer_rows_match_the_reference_outright(n, k, dim):
    rng = np.random.default_rng(1000 * n + 10 * k + dim)
    X, C = ints(rng, (n, dim)), ints(rng, (k, dim))
    C[-1] = C[0]                                     # a duplicate centroid: the lower id wins
    if n > 2:
        X[1, dim // 2] = np.nan                      # label -1, in no sum
    Xd, Cd = dev_rows(X), dev_rows(C)
    label, dist2 = host(*K.kmeans_assign(Xd, Cd))
    want_label, want_d2, _ = kmeans_ref.assign_ref(X, C)
    assert np.array_equal(label, want_label) and (k == 1 or not (label == k - 1).any())
    assert np.array_equal(dist2, want_d2.astype(np.float32), equal_nan=True)
    cent, count = host(*K.kmeans_update(Xd, torch.from_numpy(want_label).to(DEV), Cd))
    want_c, want_count = kmeans_ref.update_ref(X, want_label, C)
    assert np.array_equal(count, want_count) and np.array_equal(cent, want_c)
    if k <= 129 and n < 2000:
        u = rng.random(k)
        assert np.array_equal(K.kmeans_seed(Xd, k, torch.from_numpy(u).to(DEV))[0].cpu().numpy(), kmeans_ref.seed_ref(X, k, u))


@pytest.mark.parametrize("sizes", [[0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1], [0, 5 * CHUNK + 7, 0]])
def test_update_at_the_chunk_edges_empty_and_single_clusters(sizes):
    rng = np.random.default_rng(len(sizes))
    label = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    X, C = ints(rng, (len(label), 33)), ints(rng, (len(sizes), 33))
    for unit in (False, True):
        cent, count = host(*K.kmeans_update(dev_rows(X), torch.from_numpy(label).to(DEV), dev_rows(C), unit_centroids=unit))
        want_c, want_count = kmeans_ref.update_ref(X, label, C, unit)
        assert np.array_equal(count, want_count) and np.array_equal(count, sizes)
        assert np.array_equal(cent[count == 0], C[count == 0])          # an empty cluster keeps its centroid
        if unit:   # (the means themselves were compared outright above: what is left is the division by the float64 norm)
            assert (np.abs(cent - want_c) <= 2 * np.spacing(np.abs(want_c))).all()
        else:
            assert np.array_equal(cent, want_c)
    zero = np.concatenate([X[:4], -X[:4]])   # a mean without direction under unit_centroids: the centroid stays, count 0
    cent, count = host(*K.kmeans_update(dev_rows(zero), torch.zeros(8, dtype=torch.int32, device=DEV), dev_rows(C[:1]), unit_centroids=True))
    assert count.tolist() == [0] and np.array_equal(cent, C[:1])


def test_seed_on_a_prefix_boundary_and_on_identical_rows():
    X = np.array([[0], [1], [1], [1], [1]], np.float32)        # d = 0 1 1 1 1, T = 4, u T = 1 exactly: P_i > 1 first at row 2
    u = np.array([0.0, 0.25, 0.5, 0.99])
    ids, cent = host(*K.kmeans_seed(dev_rows(X), 4, torch.from_numpy(u).to(DEV)))
    assert ids.tolist() == kmeans_ref.seed_ref(X, 4, u).tolist() and ids[:2].tolist() == [0, 2] and np.array_equal(cent, X[ids])
    same = np.full((7, 5), 3.0, np.float32)                    # T = 0: the lowest ids not chosen yet
    u = np.array([0.5, 0.9, 0.1, 0.7, 0.3, 0.2, 0.6])
    assert K.kmeans_seed(dev_rows(same), 7, torch.from_numpy(u).to(DEV))[0].tolist() == [3, 0, 1, 2, 4, 5, 6]
    same[3, 1] = np.nan   # centre 0 falls on a row with a NaN: the next row without one
    assert K.kmeans_seed(dev_rows(same), 7, torch.from_numpy(u).to(DEV))[0].tolist() == kmeans_ref.seed_ref(same, 7, u).tolist() == [4, 0, 1, 2, 3, 5, 6]


@pytest.mark.parametrize("n, k, dim", [(257, 129, 100), (1025, 300, 33), (32801, 33, 5)])
def test_normal_rows_stay_within_the_float32_band(n, k, dim):
    rng = np.random.default_rng(n + k)
    X, C = rng.normal(size=(n, dim)).astype(np.float32), rng.normal(size=(k, dim)).astype(np.float32)
    Xd, Cd = dev_rows(X), dev_rows(C)
    label, dist2 = host(*K.kmeans_assign(Xd, Cd))
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    d2 = (X64 * X64).sum(1)[:, None] + (C64 * C64).sum(1)[None, :] - 2 * X64 @ C64.T
    tol2 = gamma(dim + 2) * ((X64 * X64).sum(1)[:, None] + (C64 * C64).sum(1)[None, :] + 2 * np.abs(X64) @ np.abs(C64).T)
    rows = np.arange(n)
    assert (label >= 0).all() and (d2[rows, label][:, None] <= d2 + tol2[rows, label][:, None] + tol2).all()
    direct = ((X64 - C64[label]) ** 2).sum(1)
    assert (np.abs(dist2 - direct) <= gamma(dim + 2) * direct).all()
    cent, count = host(*K.kmeans_update(Xd, torch.from_numpy(label).to(DEV), Cd))
    assert np.array_equal(count, np.bincount(label, minlength=k))
    live = count > 0
    mean = np.stack([X64[label == c].sum(0) for c in range(k)])[live] / count[live, None]
    mass = np.stack([np.abs(X64[label == c]).sum(0) for c in range(k)])[live] / count[live, None]
    assert (np.abs(cent[live] - mean) <= gamma(CHUNK + 1) * mass + U * np.abs(mean)).all()
    assert np.array_equal(cent[~live], C[~live])


@pytest.mark.parametrize("exact", [False, True])
def test_run_matches_the_float64_lloyd_and_is_the_same_in_one_call_or_two(exact):
    """Six blobs from one row per blob (2 iterations); integer rows, two of them with a NaN, from rows 10..16 (12 iterations, every
    decision of the float64 Lloyd at least 1e-3 clear of a tie): labels, counts, state and centroids equal the restatement outright."""
    if exact:
        X, start = ints(np.random.default_rng(3), (300, 5)), slice(10, 17)
        X[7, 2] = X[140, 0] = np.nan
    else:
        X, start = tsne_ref.clustered(300, 50, clusters=6, seed=5, centre_scale=3.0)[0], slice(0, 6)   # (row i belongs to blob i % 6)
    Xd = dev_rows(X)
    want_c, want_label, want_d2, want_count, want_inertia, want_state = kmeans_ref.run_ref(X, X[start], 50)
    def run(iters, resume=None, cent=None):
        cent = dev_rows(X[start]).contiguous() if cent is None else cent
        return K.kmeans_run(Xd, cent, iters, resume=resume)

    full = run(50)
    assert np.array_equal(full.label.cpu().numpy(), want_label) and (exact or np.array_equal(want_label, np.arange(300) % 6))
    assert full.state.tolist() == want_state.tolist() == [1, 12 if exact else 2, 0, 2 if exact else 0] and np.array_equal(full.count.cpu().numpy(), want_count)
    X64, cent = X.astype(np.float64), full.centroids.cpu().numpy()
    mean = np.stack([X64[want_label == c].mean(0) for c in range(len(cent))])
    mass = np.stack([np.abs(X64[want_label == c]).mean(0) for c in range(len(cent))])
    assert (np.abs(cent - mean) <= gamma(CHUNK + 1) * mass + U * np.abs(mean)).all() and (not exact or np.array_equal(cent, want_c))
    assert abs(full.inertia.item() - want_inertia) <= 1e-6 * want_inertia
    again, seven, three, one = run(50), run(7), run(3), run(1)
    if exact:   # the first assign is against integer centroids: dist2 and the inertia without the NaN rows are exact
        assert one.inertia.item() == kmeans_ref.run_ref(X, X[start], 1)[4] and one.state.tolist() == [0, 1, 300, 2]
    both = run(4, resume=three, cent=three.centroids)
    beyond = run(40, resume=seven, cent=seven.centroids)       # max_iter beyond convergence: nothing is written behind it
    for a, b in ((full, again), (run(7), both), (run(2), run(1, resume=one, cent=one.centroids)), (full, beyond)):
        for name in ("centroids", "label", "dist2", "count", "inertia", "state"):
            assert torch.equal(getattr(a, name).view(torch.uint8), getattr(b, name).view(torch.uint8)), name


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_cluster_entities_and_vectors_recover_the_blobs(metric):
    from pykg2vec_amd.evaluator import Evaluator
    from pykg2vec_amd.trainer import Trainer
    from test_hip_tsne import _model
    X, blob = tsne_ref.clustered(300, 50, clusters=6, seed=5, centre_scale=3.0)   # (row i belongs to blob i % 6)
    m, cfg = _model("transe", 300, 11, 50, dict(ent_embeddings=X))
    ev = Evaluator(m, cfg)
    # seed 1: by the restatement one of the two runs ends in a worse optimum under either metric; the one of lowest inertia is kept
    for labels, cent in (ev.cluster_entities(6, metric=metric, n_init=2, seed=1), ev.cluster_vectors(torch.from_numpy(X), 6, metric=metric, n_init=2, seed=1)):
        assert labels.dtype == torch.int64 and labels.is_cuda and tuple(cent.shape) == (6, 50) and cent.dtype == torch.float32
        pairs = set(zip(blob.tolist(), labels.tolist()))
        assert len(pairs) == 6 and len({b for b, _ in pairs}) == 6 and len({c for _, c in pairs}) == 6     # a bijection blob <-> label
        last = ev.last_clustering
        assert last["converged"] and last["iterations"] >= 1 and last["invalid_rows"] == 0 and last["inertia"] > 0
        assert last["counts"].tolist() == [50] * 6
        if metric == "cosine":
            assert torch.allclose(cent.norm(dim=1), torch.ones(6, device=DEV), atol=1e-6)
    tr = Trainer(m, cfg)
    tr.build_model()
    got, names = tr.cluster_entities(2, ids=[5, 2, 44, 9], metric=metric)
    assert got.shape == (4,) and got.dtype == np.int64 and names == {i: "e%d" % i for i in (5, 2, 44, 9)}
