"""kge_pca_fit / kge_pca_transform (csrc/kge_pca.hip) against the numpy float64 restatement of their contract (tests/pca_ref.py), on
strided rows whose padding holds NaN, under PCA_SPLIT = 1 and 3.  Exact cases: integer rows in -8..8 as pairs x, -x (a zero row for
an odd count, two non-finite rows from n = 5 on): every mean is 0 and every product and sum an integer below 2^53, so mean, count
and cov equal the reference outright in ANY order.  Gap-free checks, u = 2^-53, T = trace(cov_ref), tol = (n + 32 dim) dim u T: Weyl's
bound on a Gram error of gamma_n per entry plus a Jacobi backward error of a few dim u |A|; 32 is headroom for the sweep count
(DESIGN.md section 38).  Planted spectrum: rows Z diag(s) Q, Z with centred orthonormal columns, s a ladder of ratio 1.25; the test
first asserts on the CPU that the reference's relative gaps are at least 0.1 (a condition on the inputs); an axis may then differ from
the reference's by tol / (min gap T), and a projection by 2^-24 |y| plus what the axis error moves."""
import numpy as np
import pytest

from pca_ref import pca_ref, transform_ref
from test_hip_silhouette import dev_rows   # strided device rows whose padding holds NaN
from pykg2vec_amd import kernels as K

pytestmark = pytest.mark.gpu

U, U32 = 2.0 ** -53, 2.0 ** -24
FIELDS = ("mean", "cov", "explained_variance", "components", "count", "sweeps")


def fit(X, split):
    K.set_switch("PCA_SPLIT", split)
    try:
        res = K.pca_fit(dev_rows(X))
        return res, {name: getattr(res, name).cpu().numpy() for name in FIELDS}
    finally:
        K.set_switch("PCA_SPLIT", None)


def integer_rows(n, dim, rng):
    valid = n - 2 if n >= 5 else n
    half = rng.integers(-8, 9, (valid // 2, dim))
    X = np.concatenate([half, -half, np.zeros((valid % 2, dim), np.int64)]).astype(np.float32)
    if n >= 5:
        X = np.insert(X, [1, len(X)], 1.0, 0)
        X[1, dim // 2], X[-1, 0] = np.nan, np.inf
    return X


def check_gap_free(got, ref, n, dim):   # what holds whatever the gaps are; -> tol
    mean, cov, lam_ref, _, count = ref
    lam, W, sweeps = got["explained_variance"], got["components"], int(got["sweeps"][0])
    tol = (n + 32 * dim) * dim * U * np.trace(cov)
    print(dim, n, "sweeps", sweeps, "lam", np.abs(lam - lam_ref).max(), "orth / dim u", np.abs(W @ W.T - np.eye(dim)).max() / (dim * U), "tol", tol)
    assert (np.diff(lam) <= 0).all() and (lam >= 0).all() and np.abs(lam - lam_ref).max() <= tol
    assert np.abs(W @ W.T - np.eye(dim)).max() <= 32 * dim * U and np.abs(W.T @ np.diag(lam) @ W - cov).max() <= tol
    assert (W[np.arange(dim), np.abs(W).argmax(1)] > 0).all() and 1 <= sweeps <= 60
    return tol


CASES = [(n, dim) for dim in (1, 2, 15, 16, 17, 33, 65, 130) for n in (2, 3, 63, 64, 65, 257)] + [(600, K.PCA_MAX_DIM)]   # n < dim: rank-deficient


@pytest.mark.parametrize("n, dim", CASES)
def test_integer_rows_give_the_exact_covariance_and_a_backward_stable_spectrum(n, dim):
    X = integer_rows(n, dim, np.random.default_rng(1000 * n + dim))
    ref = pca_ref(X)
    for split in (1, 3) if dim < K.PCA_MAX_DIM else (None,):
        _, got = fit(X, split)
        assert got["count"][0] == ref[4] == (n - 2 if n >= 5 else n) and np.array_equal(got["mean"], ref[0]) and np.array_equal(got["cov"], ref[1])
        assert np.array_equal(got["cov"] * max(ref[4] - 1, 1), ref[1] * max(ref[4] - 1, 1)) and np.array_equal(got["cov"], got["cov"].T)
        check_gap_free(got, ref, n, dim)


LONE = np.where(np.arange(3)[:, None] == 1, np.arange(1.0, 6.0), np.nan)   # one valid row between two NaN rows
EDGES = {"equal": (np.full((70, 9), 3.0), 70), "lone": (LONE, 1), "isotropic": (2.0 * np.concatenate([np.eye(20), -np.eye(20)]), 40)}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_rows_without_variance_one_valid_row_and_an_isotropic_set(name):
    (X, count), (n, dim) = EDGES[name], EDGES[name][0].shape
    ref = pca_ref(X)
    for split in (1, 3):
        _, got = fit(X, split)
        assert got["count"][0] == count and np.array_equal(got["mean"], ref[0]) and np.array_equal(got["cov"], ref[1])
        check_gap_free(got, ref, n, dim)
        assert name == "isotropic" or not (got["cov"].any() or got["explained_variance"].any())
        assert np.array_equal(got["components"], np.eye(dim)) and got["sweeps"][0] == 1   # a diagonal matrix: nothing to rotate


@pytest.fixture(scope="module", params=[6, 12])
def planted(request):
    dim, n = request.param, 300
    rng = np.random.default_rng(dim)
    Z, Q = rng.normal(size=(n - 2, dim)), np.linalg.qr(rng.normal(size=(dim, dim)))[0]
    Z = np.linalg.qr(Z - Z.mean(0))[0]
    X = ((Z * 1.25 ** -np.arange(dim)) @ Q * 40.0 + rng.normal(size=dim)).astype(np.float32)
    X = np.insert(X, [7, 200], 0.5, 0)
    X[7, 1], X[201, dim - 1] = np.nan, -np.inf
    ref = pca_ref(X)
    gap = (1.0 - ref[2][1:] / ref[2][:-1]).min()
    assert gap >= 0.1        # a condition on the inputs
    return X, ref, gap


def test_planted_axes_and_projections_match_the_reference(planted):
    (X, ref, gap), (n, dim) = planted, planted[0].shape
    mean, cov, lam_ref, W_ref, _ = ref
    for split in (1, 3):
        res, got = fit(X, split)
        tol = check_gap_free(got, ref, n, dim)
        axis = tol / (gap * np.trace(cov))
        assert np.abs(got["components"] - W_ref).max() <= axis
        reach = np.abs(np.where(np.isfinite(X), X, 0.0) - mean).sum(1, keepdims=True)   # |x - mean|_1: what an axis error moves
        for whiten in (False, True):
            for nc in (1, 2, dim):
                Y = K.pca_transform(dev_rows(X), res, nc, whiten).cpu().numpy().astype(np.float64)
                want = transform_ref(X, mean, W_ref, lam_ref, nc, whiten)
                sd = np.sqrt(lam_ref[:nc]) if whiten else np.ones(nc)
                bound = U32 * np.abs(want) + (reach * axis + np.abs(mean).sum() * n * U) / sd + (np.abs(want) * tol / lam_ref[:nc] if whiten else 0)
                ok = np.isfinite(want)
                assert not ok[[7, 201]].any() and np.isnan(Y[[7, 201]]).all() and np.isfinite(Y[ok]).all()
                assert (np.abs(Y - want)[ok] <= bound[ok]).all(), (split, whiten, nc)


@pytest.mark.parametrize("nc", [1, 17, 130])
def test_transform_of_rows_outside_the_fit_at_the_tile_edges(nc):   # the reference takes the device's own fit: float32 rounding only
    rng = np.random.default_rng(nc)
    res, got = fit(integer_rows(65, 130, rng), None)
    lam = got["explained_variance"]
    other = rng.normal(size=(131, 130)).astype(np.float32)
    other[64, 129] = np.nan
    for whiten in (False, True):
        Y = K.pca_transform(dev_rows(other), res, nc, whiten).cpu().numpy().astype(np.float64)
        want = transform_ref(other, got["mean"], got["components"], lam, nc, whiten)
        sd = np.where(lam[:nc] > 0, np.sqrt(lam[:nc]), 1.0) if whiten else np.ones(nc)
        work = np.abs(np.where(np.isfinite(other), other, 0.0) - got["mean"]) @ np.abs(got["components"][:nc]).T
        bound = U32 * np.abs(want) + 4 * 130 * U * work / sd
        ok = np.arange(131) != 64
        assert np.isnan(Y[64]).all() and (np.abs(Y - want)[ok] <= bound[ok]).all() and (not whiten or (Y[ok][:, lam[:nc] == 0] == 0).all())

