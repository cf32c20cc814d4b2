"""kge_tsne_* (csrc/kge_tsne.hip) and the projection built on it against the numpy restatement of the contract (tests/tsne_ref.py).

Tolerances.  The perplexity search stops inside |H - log perplexity| <= 1e-5 on both sides; that band moves p by at most 1.2e-5 of the
row's maximum (measured in float64 at (n, perplexity) = (130, 30), (600, 30), (600, 5), (600, 42), (66, 2)), so p is held to 3e-5 of
the row maximum and H, evaluated in float64 from the returned float32 p, to 3e-5.  For the gradient and the descent there is no
figure to take from anywhere for float32 t-SNE, so the yardstick is computed here: the same formulas in numpy float32
(tsne_ref.gradient_ref / descent_ref with dtype=np.float32) against float64.  The device may be 4 x as far from float64 as that (a
different summation order than numpy's pairwise sums), and is never asked for less than 1e-6 of the largest component.  Figures
seen on the device are in DESIGN.md section 32."""
import functools

import numpy as np
import pytest
import torch

import hip_util
import tsne_ref
from golden_util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = 256     # KGE_TSNE_TILE


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def K():
    from pykg2vec_amd import kernels
    return kernels


# ------------------------------------------------------------------------------------------------------------------- affinities
def _affinity_rows(k, n=70, seed=0):
    """(dist float32 [n, k] ascending rows, count int32 [n]): short rows (count 1 included), a row of identical distances, rows
    scaled by 1e3 (the min-shift matters) and by 1e-3 (beta doubles many times), rows whose count is below the perplexity."""
    rng = np.random.default_rng(seed + k)
    dist = np.sort(np.abs(rng.normal(3.0, 1.0, (n, k))) + 0.1, 1).astype(np.float32)
    count = np.full(n, k, np.int32)
    count[0] = 1
    count[1] = max(1, k // 2)
    count[2] = max(1, k - 1)
    dist[3] = dist[3, 0]
    dist[4:14] *= np.float32(1e3)
    dist[14:24] *= np.float32(1e-3)
    count[24:30] = np.maximum(1, (np.arange(6) * k) // 16)          # up to 5 k / 16: below the perplexity of k / 3 for the larger k
    count[5], count[15] = max(1, k // 3 - 1), max(1, k // 4)       # (strictly below: at count == perplexity p is ill-conditioned)
    return dist, count


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128])
def test_affinities_hold_the_perplexity_and_match_the_float64_search(k):
    n = 70
    perplexity = max(1.0, k / 3)
    dist, count = _affinity_rows(k, n)
    ids = np.tile(np.arange(k, dtype=np.int32), (n, 1))
    args = (dev(ids, torch.int32), dev(dist, torch.float32), dev(count, torch.int32), perplexity)
    p_dev, beta = K().tsne_affinities(*args)
    p2, beta2 = K().tsne_affinities(*args)
    assert torch.equal(p_dev, p2) and torch.equal(beta, beta2)                     # identical bits
    p = p_dev.cpu().numpy()
    assert p.dtype == np.float32 and p.shape == (n, k) and np.isfinite(p).all() and np.isfinite(beta.cpu().numpy()).all()
    want, _ = tsne_ref.cond_p_ref(dist.astype(np.float64) ** 2, count, perplexity, tol=1e-10)
    worst = dict(sum=0.0, H=0.0, p=0.0)
    for i in range(n):
        c = int(count[i])
        assert (p[i, c:] == 0).all(), i                                            # padding places are exactly 0
        live = p[i, :c].astype(np.float64)
        worst["sum"] = max(worst["sum"], abs(live.sum() - 1.0))
        assert abs(live.sum() - 1.0) <= k * 2.0 ** -23, (i, live.sum())
        flat = np.ptp(dist[i, :c]) == 0
        assert c != perplexity or c == 1
        if c <= perplexity or flat:
            # the entropy is out of reach (log c <= log perplexity, or p is uniform whatever beta is): uniform over the live places
            assert np.abs(live - 1.0 / c).max() <= 2.0 ** -23 / c * 4, (i, c, live)
            assert np.abs(want[i, :c] - 1.0 / c).max() <= 1e-12                    # as the oracle's
            continue
        H = -(live[live > 0] * np.log(live[live > 0])).sum()
        worst["H"] = max(worst["H"], abs(H - np.log(perplexity)))
        assert abs(H - np.log(perplexity)) <= 3e-5, (i, c, H, np.log(perplexity))
        err = np.abs(live - want[i, :c]).max() / want[i, :c].max()
        worst["p"] = max(worst["p"], err)
        assert err <= 3e-5, (i, c, err)
    print("k", k, "worst |sum - 1| %.3g  |H - log perplexity| %.3g  |p - ref| / max %.3g" % (worst["sum"], worst["H"], worst["p"]))
    for key, v in worst.items():
        hip_util.record_max("tsne_edges", "affinities_k%d_%s" % (k, key), v)


# -------------------------------------------------------------------------------------------------------------------- joint CSR
@functools.lru_cache(maxsize=None)
def _device_pipeline(n, k, d=8, seed=1):
    """(X, ids, cond_p, count, csr) of a seeded clustered table through the search, the affinities and the joint on the device."""
    X, labels = tsne_ref.clustered(n, d, seed=seed)
    Xd = dev(X, torch.float32)
    own = torch.arange(n, dtype=torch.int64, device=DEV)
    ids, dist, count = K().knn_rows(Xd, Xd, k, metric="l2", self_ids=own)
    cond_p, _ = K().tsne_affinities(ids, dist, count, max(1.0, k / 3))
    return X, ids, cond_p, count, K().tsne_joint(ids, cond_p, count)


@pytest.mark.parametrize("n, k", [(130, 90), (300, 15)])
def test_joint_csr_is_the_symmetrised_union(n, k):
    X, ids, cond_p, count, csr = _device_pipeline(n, k)
    ro, col, val = csr.row_off.cpu().numpy(), csr.col.cpu().numpy(), csr.val.cpu().numpy()
    assert csr.n == n and ro.shape == (n + 1,) and ro[0] == 0 and ro[-1] == csr.nnz == len(col) == len(val)
    assert (np.diff(ro) >= 0).all()                                                # monotone offsets
    for i in range(n):
        c = col[ro[i]:ro[i + 1]]
        assert (np.diff(c) > 0).all() and i not in c and c.min() >= 0 and c.max() < n       # ascending, no duplicate, no diagonal
    got = tsne_ref.dense_of(ro, col, val, n)
    want = tsne_ref.joint_ref(ids.cpu().numpy(), cond_p.cpu().numpy(), count.cpu().numpy())
    ulp = np.spacing(np.maximum(np.abs(want), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= 4 * ulp).all(), np.abs((got - want) / ulp).max()
    assert np.array_equal(got, got.T)                                              # symmetric bit for bit
    assert abs(got.sum() - 1.0) <= 1e-6, got.sum()
    again = K().tsne_joint(ids, cond_p, count)
    assert all(torch.equal(a, b) for a, b in zip(csr[:3], again[:3]))


# --------------------------------------------------------------------------------------------------------------------- gradient
@functools.lru_cache(maxsize=None)
def _problem(n):
    """(P float64 [n, n] holding float32 values, csr on the device): the joint probabilities of a seeded clustered table at the
    library's neighbour count, from the restatement; both sides see the float32 values of the CSR."""
    X, _ = tsne_ref.clustered(n, 8, seed=n)
    perplexity = min(30.0, max(1.0, (n - 1) / 3.0))
    ro, col, val = tsne_ref.csr_of(tsne_ref.dense_P(X, perplexity))
    csr = K().TsneCSR(dev(ro, torch.int64), dev(col, torch.int32), dev(val, torch.float32), n)
    return tsne_ref.dense_of(ro, col, val, n), csr


@functools.lru_cache(maxsize=None)
def _maps(n):
    """The four maps of the gradient test, float32 [n, 2] each."""
    rng = np.random.default_rng(100 + n)
    init = rng.normal(0.0, 1e-4, (n, 2)).astype(np.float32)                        # every w ~ 1, Z ~ n (n - 1), P - Q cancels
    if n <= 257:
        P, _ = _problem(n)
        lr = max(n / 12.0 / 4.0, 50.0)
        trained = tsne_ref.descent_ref(P, init, 100, 12.0, 0.5, lr)[0].astype(np.float32)    # a trained map
    else:
        trained = rng.uniform(-30.0, 30.0, (n, 2)).astype(np.float32)
    coincident = trained.copy()
    same = rng.choice(n, min(8, n - 1), replace=False)                              # eight exactly coincident points (fewer below 9)
    coincident[same] = coincident[same[0]]
    far = trained.copy()
    far[n // 2] = (1e4, -1e4)                                                       # one point at 1e4
    return dict(init=init, trained=trained, coincident=coincident, far=far)


def _check_gradient(n, split, monkeypatch):
    if split is None:
        monkeypatch.delenv("KGE_TSNE_SPLIT", raising=False)
    else:
        monkeypatch.setenv("KGE_TSNE_SPLIT", split)
    P, csr = _problem(n)
    for name, Y in _maps(n).items():
        Yd = dev(Y, torch.float32)
        for exaggeration in (1.0, 12.0):
            g64, Z64, KL64 = tsne_ref.gradient_ref(P, Y, exaggeration)
            g32, _, _ = tsne_ref.gradient_ref(P, Y, exaggeration, dtype=np.float32)
            scale = np.abs(g64).max()
            if n == 2 and exaggeration == 1.0:
                # two points: P_01 = Q_01 = 1/2 on every map, the gradient is identically zero and grad64 is rounding noise.  The
                # two terms that cancel are the scale there: 4 P w |y_0 - y_1|.
                scale = 4 * 0.5 * np.abs(Y[0].astype(np.float64) - Y[1]).max() / (1 + ((Y[0].astype(np.float64) - Y[1]) ** 2).sum())
            yard = np.abs(g32 - g64).max() / scale
            grad, Z, KL = K().tsne_gradient(csr, Yd, exaggeration, want_kl=True)
            g = grad.cpu().numpy()
            assert g.dtype == np.float32 and g.shape == (n, 2) and np.isfinite(g).all(), (n, name)
            err = np.abs(g - g64).max() / scale
            zerr, klerr = abs(Z.item() - Z64) / Z64, abs(KL.item() - KL64)
            print("n %d split %s map %s exaggeration %g: err %.3g  float32 yardstick %.3g  Z rel %.3g  KL abs %.3g"
                  % (n, split, name, exaggeration, err, yard, zerr, klerr))
            hip_util.record_max("tsne_edges", "gradient_n%d_%s_err_over_yardstick" % (n, name), err / max(yard, 2.5e-7))
            hip_util.record_max("tsne_edges", "gradient_n%d_%s_err" % (n, name), err)
            assert err <= max(4 * yard, 1e-6), (n, split, name, exaggeration, err, yard)
            assert zerr <= 1e-6, (n, split, name, Z.item(), Z64)
            assert klerr <= 1e-5, (n, split, name, KL.item(), KL64)
            grad2, Z2, KL2 = K().tsne_gradient(csr, Yd, exaggeration, want_kl=True)          # the same bits at the same S
            assert torch.equal(grad, grad2) and torch.equal(Z, Z2) and torch.equal(KL, KL2)
            g0, Z0, none = K().tsne_gradient(csr, Yd, exaggeration)                           # KL only when asked for
            assert none is None and torch.equal(g0, grad) and torch.equal(Z0, Z)


@pytest.mark.parametrize("n", sorted({2, 3, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1, 1000}))
def test_gradient_against_float64_within_the_float32_yardstick(n, monkeypatch):
    _check_gradient(n, None, monkeypatch)


@pytest.mark.parametrize("n, split", [(1000, "1"), (1000, "3"), (1000, "64"), (1300, "3")])
def test_gradient_at_forced_slab_splits(n, split, monkeypatch):
    """1 000 points are four tiles: TSNE_SPLIT 1 -> one slab, 3 -> two slabs of two tiles, 64 -> its maximum of four; 1 300
    points are six tiles: 3 -> three slabs.  Across S the summation order differs: the tolerance holds, not the bits."""
    _check_gradient(n, split, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------- descent
def test_descent_matches_float64_and_is_the_same_in_one_call_or_two():
    n, k, iters = 200, 90, 20
    X, _ = tsne_ref.clustered(n, 8, seed=7)
    ro, col, val = tsne_ref.csr_of(tsne_ref.dense_P(X, k / 3.0))
    P = tsne_ref.dense_of(ro, col, val, n)
    csr = K().TsneCSR(dev(ro, torch.int64), dev(col, torch.int32), dev(val, torch.float32), n)
    Y0 = np.random.default_rng(11).normal(0.0, 1e-4, (n, 2)).astype(np.float32)
    kw = dict(exaggeration=12.0, momentum=0.5, learning_rate=50.0)
    ref64 = tsne_ref.descent_ref(P, Y0, iters, dtype=np.float64, record_every=10, **kw)
    ref32 = tsne_ref.descent_ref(P, Y0, iters, dtype=np.float32, record_every=10, **kw)

    def run(cuts):
        Y = dev(Y0, torch.float32)
        update, gains = K().tsne_state(Y)
        trace, it = torch.full((iters // 10, 2), float("nan"), dtype=torch.float64, device=DEV), 0
        for m in cuts:
            Y, trace = K().tsne_run(csr, Y, m, it0=it, record_every=10, update=update, gains=gains, trace=trace, **kw)
            it += m
        return Y, update, gains, trace

    one, two = run([20]), run([10, 10])
    for a, b in zip(one, two):
        assert torch.equal(a, b)                                                   # all of the state is in the caller's buffers
    for name, got, r64, r32 in zip(("Y", "update", "gains"), one[:3], ref64[:3], ref32[:3]):
        got = got.cpu().numpy()
        scale = np.abs(r64).max()
        yard, err = np.abs(r32 - r64).max(), np.abs(got - r64).max()
        print("%s: err %.3g  float32 yardstick %.3g  scale %.3g" % (name, err, yard, scale))
        hip_util.record_max("tsne_edges", "descent_%s_err_over_scale" % name, err / scale)
        assert np.isfinite(got).all() and err <= max(4 * yard, 1e-6 * scale), (name, err, yard, scale)
    assert one[2].min().item() >= 0.01                                             # gains never go below 0.01
    trace = one[3].cpu().numpy()
    assert trace.shape == (2, 2) and np.isfinite(trace).all()
    assert np.abs(trace[:, 0] - ref64[3][:, 0]).max() <= 1e-4 and np.allclose(trace[:, 1], ref64[3][:, 1], rtol=1e-3)
    # the first record is KL and |grad| of the map iteration 9 started from: tsne_gradient's on the same Y, bit for bit
    Y9 = run([9])[0]
    grad, _, KL = K().tsne_gradient(csr, Y9, 12.0, want_kl=True)
    assert KL.item() == trace[0, 0]
    assert abs(np.sqrt((grad.double() ** 2).sum().item()) - trace[0, 1]) <= 1e-12 * trace[0, 1]
    # record_every = 0: no trace is needed
    Y, tr = K().tsne_run(csr, dev(Y0, torch.float32), 3, **kw)
    assert tr.numel() == 0 and torch.isfinite(Y).all()


# -------------------------------------------------------------------------------------------------------------------- end to end
def _model(name, E, R, d, tables, seed=0):
    import kge_oracle as ko
    rng = np.random.default_rng(seed)
    hp = dict(hidden_size=d, l1_flag=True, margin=1.0)
    params = ko.init_params(name, rng, tot_entity=E, tot_relation=R, hidden_size=d)
    params.update(tables)
    trip = np.stack([rng.integers(E, size=400), rng.integers(R, size=400), rng.integers(E, size=400)], 1)
    cfg = hip_util.make_config(E, R, hp, trip[:300], trip[300:350], trip[350:], disp_triple_num=12)
    cfg.knowledge_graph.cache.update(idx2entity={i: "e%d" % i for i in range(E)}, idx2relation={i: "r%d" % i for i in range(R)})
    return hip_util.model_from_params(name, params, hp, E, R), cfg


def test_project_entities_separates_gaussian_clusters():
    from pykg2vec_amd.evaluator import Evaluator
    from pykg2vec_amd.visualization import Visualization
    E, d = 300, 50
    X, labels = tsne_ref.clustered(E, d, clusters=6, seed=5, centre_scale=3.0)
    m, cfg = _model("transe", E, 11, d, dict(ent_embeddings=X))
    ev = Evaluator(m, cfg)
    kw = dict(perplexity=30.0, n_iter=500, init="random", seed=3)
    Y = ev.project_entities(**kw)
    trace = ev.last_projection_trace.cpu().numpy()
    assert Y.dtype == torch.float32 and tuple(Y.shape) == (E, 2) and Y.is_cuda and torch.isfinite(Y).all()
    assert trace.shape == (10, 2) and np.isfinite(trace).all()
    assert trace[-1, 0] < trace[0, 0]                                              # the final recorded KL is below the first
    y = Y.cpu().numpy().astype(np.float64)
    D = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    D[np.arange(E), np.arange(E)] = np.inf
    nn = np.argsort(D, 1)[:, :10]
    purity = (labels[nn] == labels[:, None]).mean(1)
    print("10-neighbour purity: min %.2f mean %.4f" % (purity.min(), purity.mean()))
    assert purity.min() >= 0.95, np.sort(purity)[:5]
    # the float64 descent of the restatement on the same P and the same init
    table = m.entity_matrix()
    own = torch.arange(E, dtype=torch.int64, device=DEV)
    ids, dist, count = K().knn_rows(table, table, 90, metric="l2", self_ids=own)
    csr = K().tsne_joint(ids, K().tsne_affinities(ids, dist, count, 30.0)[0], count)
    P = tsne_ref.dense_of(csr.row_off.cpu().numpy(), csr.col.cpu().numpy(), csr.val.cpu().numpy(), E)
    Y0 = ev._projection_init(table, "random", 3).cpu().numpy()
    lr = max(E / 12.0 / 4.0, 50.0)
    y1, u1, g1, t1 = tsne_ref.descent_ref(P, Y0, 250, 12.0, 0.5, lr, record_every=50)
    _, _, _, t2 = tsne_ref.descent_ref(P, y1, 250, 1.0, 0.8, lr, u1, g1, record_every=50, it0=250)
    ratio = trace[-1, 0] / t2[-1, 0]
    print("final KL: device %.6f  float64 restatement %.6f  ratio %.4f" % (trace[-1, 0], t2[-1, 0], ratio))
    hip_util.record_max("tsne_edges", "end_to_end_kl_ratio", ratio)
    hip_util.record_max("tsne_edges", "end_to_end_kl_ratio_inverse", 1.0 / ratio)
    assert 1 / 1.25 <= ratio <= 1.25, ratio
    # the same seed, the same bits
    Y2 = ev.project_entities(**kw)
    assert torch.equal(Y, Y2) and torch.equal(ev.last_projection_trace, torch.from_numpy(trace).to(DEV))
    # Visualization on the device: the sampled triples' heads and tails
    out = Visualization(m, cfg, vis_opts={"ent_only_plot": True}, evaluator=ev).plot_embedding(algos="transe", project_only=True, n_iter=60)
    xy, names = out["transe_entity_plot"]
    assert xy.shape == (2 * cfg.disp_triple_num, 2) and len(names) == 2 * cfg.disp_triple_num and np.isfinite(xy).all()


@pytest.mark.parametrize("case", ["distmult", "complex"])
def test_project_relations_and_vectors_on_other_models(case):
    from pykg2vec_amd.evaluator import Evaluator
    c = Case(case)
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    m = hip_util.model_from_case(c)
    ev = Evaluator(m, cfg)
    Yr = ev.project_relations(perplexity=2.0, n_iter=40)
    assert tuple(Yr.shape) == (c.R, 2) and Yr.dtype == torch.float32 and Yr.is_cuda and torch.isfinite(Yr).all()
    rows = m.entity_matrix()                                                        # ComplEx: the real and imaginary tables side by side
    assert rows.shape[1] == (2 if case == "complex" else 1) * c.hp["hidden_size"]
    Yv = ev.project_vectors(torch.cat([rows[:20], rows[25:45] + 0.5]), perplexity=5.0, n_iter=40, init="pca")
    assert tuple(Yv.shape) == (40, 2) and torch.isfinite(Yv).all()
    Ye = ev.project_entities(ids=[1, 5, 9, 2, 40, 41, 42, 7], perplexity=2.0, n_iter=40)
    assert tuple(Ye.shape) == (8, 2) and torch.isfinite(Ye).all()
