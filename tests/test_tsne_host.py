"""CPU-only checks of the t-SNE projection: header, ctypes binding and exported symbols agree; every kge_tsne_* entry point refuses bad
arguments before any GPU call; kernels.tsne_joint (torch ops, any device) builds the CSR of the contract; Evaluator.project_*,
Visualization and Trainer.display / project_entities plumb neighbour count, perplexity, learning rate, init and names correctly over
an injected backend built from the numpy restatement (tests/tsne_ref.py) and the numpy search (tests/knn_ref.py); and the perplexity
search of the restatement is sklearn's."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import hip_util
import knn_ref
import oracle_backend
import tsne_ref
from golden_util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call
F = ctypes.c_float


def _aff(lib, dist=FAKE, count=FAKE, n=100, k=5, perplexity=2.0, cond_p=FAKE, beta=FAKE):
    return lib.kge_tsne_affinities(dist, count, n, k, F(perplexity), cond_p, beta, None)


def _grad(lib, Y=FAKE, n=100, row_off=FAKE, col=FAKE, val=FAKE, nnz=500, exaggeration=1.0, ws=FAKE, ws_bytes=1 << 30, grad=FAKE, Z=FAKE,
          KL=None):
    return lib.kge_tsne_gradient(Y, n, row_off, col, val, nnz, F(exaggeration), ws, ws_bytes, grad, Z, KL, None)


def _run(lib, Y=FAKE, Y_tmp=FAKE, update=FAKE, gains=FAKE, n=100, row_off=FAKE, col=FAKE, val=FAKE, nnz=500, it0=0, it1=10, exaggeration=12.0,
         momentum=0.5, learning_rate=200.0, record_every=0, trace=None, n_records=0, ws=FAKE, ws_bytes=1 << 30):
    return lib.kge_tsne_run(Y, Y_tmp, update, gains, n, row_off, col, val, nnz, it0, it1, F(exaggeration), F(momentum), F(learning_rate),
                            record_every, trace, n_records, ws, ws_bytes, None)


@pytest.mark.parametrize("call, kw, word", [
    (_aff, dict(n=1, perplexity=1.0), b"n = 1"), (_aff, dict(k=0), b"k = 0"), (_aff, dict(k=129), b"k = 129"),
    (_aff, dict(perplexity=0.5), b"perplexity"), (_aff, dict(perplexity=100.0), b"perplexity"), (_aff, dict(perplexity=math.nan), b"perplexity"),
    (_aff, dict(dist=None), b"null"), (_aff, dict(count=None), b"null"), (_aff, dict(cond_p=None), b"null"), (_aff, dict(beta=None), b"null"),
    (_grad, dict(n=1, nnz=0), b"n = 1"), (_grad, dict(nnz=-1), b"nnz"), (_grad, dict(nnz=100 * 99 + 1), b"nnz"),
    (_grad, dict(Y=None), b"null"), (_grad, dict(row_off=None), b"null"), (_grad, dict(col=None), b"null"), (_grad, dict(val=None), b"null"),
    (_grad, dict(grad=None), b"null"), (_grad, dict(Z=None), b"null"), (_grad, dict(exaggeration=0.0), b"exaggeration"),
    (_grad, dict(exaggeration=math.inf), b"exaggeration"), (_grad, dict(ws=None), b"workspace"), (_grad, dict(ws_bytes=16), b"workspace"),
    (_run, dict(n=1, nnz=0), b"n = 1"), (_run, dict(nnz=100 * 99 + 1), b"nnz"), (_run, dict(learning_rate=math.inf), b"learning_rate"),
    (_run, dict(learning_rate=math.nan), b"learning_rate"), (_run, dict(momentum=1.0), b"momentum"), (_run, dict(momentum=-0.1), b"momentum"),
    (_run, dict(momentum=math.nan), b"momentum"), (_run, dict(Y=None), b"null"), (_run, dict(Y_tmp=None), b"null"),
    (_run, dict(update=None), b"null"), (_run, dict(gains=None), b"null"), (_run, dict(row_off=None), b"null"),
    (_run, dict(it0=5, it1=4), b"iterations"), (_run, dict(record_every=-1), b"record_every"),
    (_run, dict(record_every=5, trace=None), b"trace"), (_run, dict(record_every=5, trace=FAKE, n_records=1), b"trace"),
    (_run, dict(ws=None), b"workspace"), (_run, dict(ws_bytes=16), b"workspace"),
])
def test_tsne_entry_points_refuse_bad_arguments_without_gpu(call, kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert call(lib, **kw) == -1
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_tsne_workspace_is_a_function_of_n_and_the_split(monkeypatch):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    monkeypatch.delenv("KGE_TSNE_SPLIT", raising=False)
    T = _lib.TSNE_TILE
    assert lib.kge_tsne_workspace_bytes(1) == 0            # a refused n asks for nothing
    for n in (2, T - 1, T, T + 1, 1000, 14951, 123182):
        tiles = -(-n // T)
        monkeypatch.delenv("KGE_TSNE_SPLIT", raising=False)
        auto = lib.kge_tsne_workspace_bytes(n)
        assert auto == lib.kge_tsne_workspace_bytes(n)      # nothing but n decides
        monkeypatch.setenv("KGE_TSNE_SPLIT", "1")
        one = lib.kge_tsne_workspace_bytes(n)
        assert 16 * n + 8 * tiles <= one <= 16 * n + 8 * tiles + 32768     # one (fx, fy, sum w, -) per point, one float64 per workgroup
        assert one <= auto <= 64 * (16 * n + 8 * tiles) + 32768            # at most 64 slabs
        monkeypatch.setenv("KGE_TSNE_SPLIT", "1000")
        most = lib.kge_tsne_workspace_bytes(n)
        per = -(-tiles // min(tiles, 64))                                   # whole tiles per slab, no slab empty
        assert most >= -(-tiles // per) * 16 * n and most >= auto
    # small maps are split so that they still fill the device, large ones are not
    monkeypatch.delenv("KGE_TSNE_SPLIT", raising=False)
    assert lib.kge_tsne_workspace_bytes(14951) >= 8 * 16 * 14951
    monkeypatch.setenv("KGE_TSNE_SPLIT", "1")
    one = lib.kge_tsne_workspace_bytes(1 << 20)
    monkeypatch.delenv("KGE_TSNE_SPLIT", raising=False)
    assert lib.kge_tsne_workspace_bytes(1 << 20) == one


def test_tsne_header_binding_and_constants_agree():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_TSNE_TILE\s+(\d+)", text).group(1)) == _lib.TSNE_TILE == kernels.TSNE_TILE == 256
    lib = _lib.load()
    for sym in ("kge_tsne_affinities", "kge_tsne_workspace_bytes", "kge_tsne_gradient", "kge_tsne_run"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        proto = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % sym, text, re.M).group(1)      # (the declaration, not the comment's mention)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[sym][1]), sym
    assert "TSNE_SPLIT" in text
    assert _lib.ABI_VERSION == 3   # additive entry points


def test_tsne_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from pykg2vec_amd import _lib, kernels
    ids, dist, count = torch.zeros((10, 4), dtype=torch.int32), torch.zeros((10, 4)), torch.full((10,), 4, dtype=torch.int32)
    with pytest.raises(_lib.KgeHipError):
        kernels.tsne_affinities(ids, dist, count, 2.0)
    with pytest.raises(TypeError):
        kernels.tsne_affinities(ids, dist.double(), count, 2.0)
    with pytest.raises(ValueError):
        kernels.tsne_affinities(ids[:, :3], dist, count, 2.0)
    csr = kernels.tsne_joint(torch.tensor([[1], [0]], dtype=torch.int32), torch.ones((2, 1)), torch.ones(2, dtype=torch.int32))
    with pytest.raises(_lib.KgeHipError):
        kernels.tsne_gradient(csr, torch.zeros((2, 2)))
    with pytest.raises(ValueError):
        kernels.tsne_gradient(csr, torch.zeros((3, 2)))
    with pytest.raises(_lib.KgeHipError):
        kernels.tsne_run(csr, torch.zeros((2, 2)), 1)


@pytest.mark.parametrize("n, k", [(2, 1), (40, 7), (130, 90)])
def test_tsne_joint_builds_the_csr_of_the_contract(n, k):
    from pykg2vec_amd import kernels
    X, _ = tsne_ref.clustered(n, 6, seed=n)
    ids, dist, count = tsne_ref.neighbours_l2(X, k)
    count[::5] = np.maximum(1, count[::5] // 2)                # short rows: the places behind count take no part
    p = tsne_ref.cond_p_ref(dist.astype(np.float64) ** 2, count, max(1.0, k / 3))[0].astype(np.float32)
    csr = kernels.tsne_joint(torch.from_numpy(ids), torch.from_numpy(p), torch.from_numpy(count))
    ro, col, val = csr.row_off.numpy(), csr.col.numpy(), csr.val.numpy()
    assert csr.n == n and csr.nnz == len(col) == len(val) == ro[-1] and ro[0] == 0 and ro.dtype == np.int64 and col.dtype == np.int32
    assert (np.diff(ro) >= 0).all()
    for i in range(n):
        c = col[ro[i]:ro[i + 1]]
        assert (np.diff(c) > 0).all() and i not in c and ((c >= 0) & (c < n)).all()
    want = tsne_ref.joint_ref(ids, p, count)
    got = tsne_ref.dense_of(ro, col, val, n)
    assert (got[want >= 2.0 ** -100] != 0).all() and (want[got != 0] != 0).all()      # the union graph: nothing lost, nothing added
    assert np.abs(got - want).max() <= 4 * np.spacing(np.float32(want.max()))
    assert np.array_equal(got, got.T)                          # symmetric bit for bit
    if (count >= 1).all():
        assert abs(got.sum() - 1.0) <= 1e-6


# ---------------------------------------------------------------------------------------------- plumbing over an injected backend
class Backend(tsne_ref.Backend):
    """oracle_backend (what Trainer.build_model needs on the CPU) + the numpy search + the numpy t-SNE, with the calls recorded."""

    def __init__(self):
        super().__init__(**{k: v for k, v in vars(oracle_backend).items() if not k.startswith("__")})
        self.chunks = []

    def knn_rows(self, table, queries, k, metric="cosine", self_ids=None):
        self.chunks.append((int(queries.shape[0]), int(k), metric, self_ids is not None))
        return knn_ref.knn_rows_torch(table, queries, k, metric, self_ids)


def _setup(case="transe_l1", **extra):
    c = Case(case)
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, device="cpu", **extra)
    cfg.knowledge_graph.cache.update(idx2entity={i: "e%d" % i for i in range(c.E)}, idx2relation={i: "r%d" % i for i in range(c.R)})
    m = hip_util.model_from_case(c, device="cpu")
    from pykg2vec_amd.evaluator import Evaluator
    B = Backend()
    return c, cfg, m, Evaluator(m, cfg, backend=B), B


def test_project_entities_plumbs_neighbours_learning_rate_and_phases():
    c, cfg, m, ev, B = _setup()
    Y = ev.project_entities(perplexity=5.0, n_iter=30, exaggeration_iter=20, record_every=10)
    assert Y.dtype == torch.float32 and tuple(Y.shape) == (c.E, 2) and torch.isfinite(Y).all()      # ids=None: every entity
    assert B.chunks == [(c.E, 15, "l2", True)]                                                       # floor(3 x 5) neighbours, own row excluded
    lr = max(c.E / 12.0 / 4.0, 50.0)
    assert B.calls == [("affinities", (c.E, 15), 5.0), ("run", 20, 0, 12.0, 0.5, lr, 10), ("run", 10, 20, 1.0, 0.8, lr, 10)]
    tr = ev.last_projection_trace
    assert tuple(tr.shape) == (3, 2) and torch.isfinite(tr).all()
    # the same run through the restatement alone
    W = m.entity_matrix().numpy()
    assert np.array_equal(B.P, tsne_ref.dense_P(W, 5.0))
    P = tsne_ref.dense_of(*tsne_ref.csr_of(B.P), c.E)            # (the CSR's float32 values, as the descent was handed them)
    y, u, g, t0 = tsne_ref.descent_ref(P, B.init.numpy(), 20, 12.0, 0.5, lr, record_every=10)
    y, _, _, t1 = tsne_ref.descent_ref(P, y.astype(np.float32), 10, 1.0, 0.8, lr, u.astype(np.float32), g.astype(np.float32), record_every=10, it0=20)
    assert np.array_equal(Y.numpy(), y.astype(np.float32)) and np.array_equal(tr.numpy(), np.concatenate([t0, t1]))
    # a complete graph below 3 x perplexity + 1 rows: n - 1 neighbours; ids pick rows; learning_rate given
    B.chunks.clear(), B.calls.clear()
    ids = [3, 9, 1, 40, 22, 7, 8, 30, 31, 12]
    Y = ev.project_entities(ids, perplexity=3.0, n_iter=4, exaggeration_iter=250, learning_rate=17.5, init="random", record_every=0)
    assert tuple(Y.shape) == (10, 2) and B.chunks == [(10, 9, "l2", True)]
    assert B.calls[1:] == [("run", 4, 0, 12.0, 0.5, 17.5, 0), ("run", 0, 4, 1.0, 0.8, 17.5, 0)] and ev.last_projection_trace.numel() == 0
    assert B.calls[0] == ("affinities", (10, 9), 3.0)
    for bad in (0.5, 10.0, 53.0):
        with pytest.raises(ValueError, match="perplexity"):
            ev.project_entities(ids, perplexity=bad)
    with pytest.raises(ValueError, match="at least 2"):
        ev.project_entities([4])


def test_project_refuses_more_neighbours_than_the_search_returns():
    c, cfg, m, ev, B = _setup()
    X = torch.from_numpy(tsne_ref.clustered(131, 5, seed=2)[0])
    with pytest.raises(ValueError, match=r"129 neighbours.*128 \(KGE_KNN_MAX\)"):
        ev.project_vectors(X, perplexity=43.0)
    with pytest.raises(ValueError, match="KGE_KNN_MAX"):
        ev.project_vectors(X[:130], perplexity=60.0)                # n - 1 = 129 neighbours: one more than the search returns
    assert not B.chunks and not B.calls                             # refused before anything ran
    Y = ev.project_vectors(X, perplexity=42.0, n_iter=1)            # 126 neighbours: the widest sparse graph
    assert tuple(Y.shape) == (131, 2) and B.chunks == [(131, 126, "l2", True)]


def test_project_at_129_rows_is_the_complete_graph():
    c, cfg, m, ev, B = _setup()
    X = torch.from_numpy(tsne_ref.clustered(129, 5, seed=3)[0])
    Y = ev.project_vectors(X, perplexity=60.0, n_iter=2, record_every=1)
    assert tuple(Y.shape) == (129, 2) and B.chunks == [(129, 128, "l2", True)]


def test_projection_init_pca_scale_determinism_random_and_given():
    c, cfg, m, ev, B = _setup()
    X = torch.from_numpy(tsne_ref.clustered(60, 9, seed=4)[0])
    a, b = ev._projection_init(X, "pca", 0), ev._projection_init(X, "pca", 99)
    assert a.dtype == torch.float32 and tuple(a.shape) == (60, 2) and torch.equal(a, b)
    assert abs(float(a[:, 0].double().std(unbiased=False)) - 1e-4) <= 1e-9
    # the top two principal axes: the coordinates' variances are the two largest eigenvalues, in order, and they are uncorrelated
    Xc = X.double().numpy() - X.double().numpy().mean(0)
    ev2 = np.sort(np.linalg.eigvalsh(Xc.T @ Xc / 59))[::-1]
    var = a.double().numpy().var(0, ddof=1)
    assert np.allclose(var[1] / var[0], ev2[1] / ev2[0], rtol=1e-5)
    assert abs(np.corrcoef(a.double().numpy().T)[0, 1]) < 1e-5
    r0, r1, r2 = ev._projection_init(X, "random", 0), ev._projection_init(X, "random", 0), ev._projection_init(X, "random", 1)
    assert torch.equal(r0, r1) and not torch.equal(r0, r2) and 5e-5 < float(r0.std()) < 2e-4
    given = torch.arange(120, dtype=torch.float64).view(60, 2)
    g = ev._projection_init(X, given, 0)
    assert g.dtype == torch.float32 and torch.equal(g, given.float()) and g.data_ptr() != given.data_ptr()
    with pytest.raises(ValueError):
        ev._projection_init(X, given[:5], 0)
    with pytest.raises(ValueError):
        ev._projection_init(X, "spectral", 0)


def test_project_relations_and_vectors_take_the_right_rows():
    c, cfg, m, ev, B = _setup("transh_l1")
    Y = ev.project_relations(perplexity=2.0, n_iter=3, init="random")
    assert tuple(Y.shape) == (c.R, 2) and B.chunks == [(c.R, 6, "l2", True)]
    assert B.calls[0] == ("affinities", (c.R, 6), 2.0)
    Rm = m.relation_matrix().numpy()                     # [rel_embedding | w]
    assert np.array_equal(B.P, tsne_ref.dense_P(Rm, 2.0))
    B.chunks.clear()
    ev.project_relations(tables=["w"], perplexity=2.0, n_iter=1, init="random")
    assert np.array_equal(B.P, tsne_ref.dense_P(m.w.weight.detach().numpy(), 2.0))
    rows = np.concatenate([m.entity_matrix().numpy()[:8], m.entity_matrix().numpy()[20:28]])
    Y = ev.project_vectors(rows, perplexity=4.0, n_iter=1)
    assert tuple(Y.shape) == (16, 2) and np.array_equal(B.P, tsne_ref.dense_P(rows, 4.0))
    with pytest.raises(ValueError):
        ev.project_vectors(rows[0])


def test_trainer_project_entities_returns_coordinates_and_names():
    from pykg2vec_amd.trainer import Trainer
    c, cfg, m, ev, B = _setup()
    tr = Trainer(m, cfg, backend=B)
    tr.build_model()
    coords, names = tr.project_entities([5, 2, 44, 9, 17, 3], perplexity=1.5, n_iter=2)
    assert isinstance(coords, np.ndarray) and coords.shape == (6, 2) and coords.dtype == np.float32
    assert names == {i: "e%d" % i for i in (5, 2, 44, 9, 17, 3)} and list(names) == [5, 2, 44, 9, 17, 3]
    coords, names = tr.project_entities(perplexity=4.0, n_iter=1)
    assert coords.shape == (c.E, 2) and names == {i: "e%d" % i for i in range(c.E)}


def test_visualization_clamps_the_perplexity_and_returns_names():
    from pykg2vec_amd.visualization import Visualization
    assert Visualization.perplexity_for(20) == pytest.approx(19 / 3.0)       # the reference's 20 relation points
    assert Visualization.perplexity_for(40) == pytest.approx(13.0) and Visualization.perplexity_for(1000) == 30.0
    assert Visualization.perplexity_for(2) == 1.0 and Visualization.perplexity_for(91) == 30.0
    c, cfg, m, ev, B = _setup(disp_triple_num=7)
    opts = {"ent_only_plot": True, "rel_only_plot": True, "ent_and_rel_plot": True}
    viz = Visualization(m, cfg, vis_opts=opts, evaluator=ev)
    assert len(viz.h_emb) == len(viz.r_emb) == len(viz.t_emb) == len(viz.h_name) == 7
    again = Visualization(m, cfg, vis_opts=opts, evaluator=ev)
    assert again.h_name == viz.h_name and again.r_name == viz.r_name                # sampled from config.seed
    valid = {(int(h), int(r), int(t)) for h, r, t in c.valid}
    W = m.ent_embeddings.weight.detach()
    for hn, rn, tn, he in zip(viz.h_name, viz.r_name, viz.t_name, viz.h_emb):
        assert (int(hn[1:]), int(rn[1:]), int(tn[1:])) in valid and torch.equal(he[0], W[int(hn[1:])])
    out = viz.plot_embedding(algos="TransE", project_only=True, n_iter=3)
    assert sorted(out) == ["TransE_ent_n_rel_plot", "TransE_entity_plot", "TransE_rel_plot"]
    xy, names = out["TransE_entity_plot"]
    assert xy.shape == (14, 2) and list(names) == viz.h_name + viz.t_name
    assert out["TransE_rel_plot"][0].shape == (7, 2) and out["TransE_ent_n_rel_plot"][0].shape == (21, 2)
    perps = [call[2] for call in B.calls if call[0] == "affinities"]
    assert perps == [pytest.approx(13 / 3.0), pytest.approx(2.0), pytest.approx(20 / 3.0)]
    none = Visualization(m, cfg, evaluator=ev).plot_embedding(algos="TransE", project_only=True)
    assert none == {}


def test_visualization_and_trainer_display_write_the_pngs(tmp_path):
    pytest.importorskip("matplotlib")
    from pykg2vec_amd.trainer import Trainer
    from pykg2vec_amd.visualization import Visualization
    c, cfg, m, ev, B = _setup(disp_triple_num=6)
    viz = Visualization(m, cfg, vis_opts={"ent_only_plot": True, "rel_only_plot": True, "ent_and_rel_plot": True}, evaluator=ev)
    viz.plot_embedding(resultpath=tmp_path / "a", algos="transe", show_label=True, disp_num_r_n_e=4, n_iter=2)
    for stem in ("transe_entity_plot", "transe_rel_plot", "transe_ent_n_rel_plot"):
        f = tmp_path / "a" / (stem + ".png")
        assert f.exists() and f.stat().st_size > 1000 and f.read_bytes()[:4] == b"\x89PNG"
    # Trainer.display: the reference's options from the configuration's flags
    cfg.plot_embedding, cfg.plot_entity_only, cfg.path_figures = True, True, tmp_path / "b"
    cfg.plot_training_result = cfg.plot_testing_result = True
    tr = Trainer(m, cfg, backend=B)
    tr.build_model()
    tr.display()
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["%s_entity_plot.png" % m.model_name]
    cfg.plot_entity_only, cfg.path_figures = False, tmp_path / "c"
    tr.display()
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == sorted("%s_%s.png" % (m.model_name, s) for s in
                                                                       ("entity_plot", "rel_plot", "ent_n_rel_plot"))
    cfg.plot_embedding, cfg.path_figures = False, tmp_path / "d"
    tr.display()
    assert not (tmp_path / "d").exists()


# ------------------------------------------------------------------------------------------------ the search is sklearn's
@pytest.mark.parametrize("n, perplexity", [(130, 30.0), (600, 30.0), (600, 5.0), (600, 42.0), (66, 2.0)])
def test_cond_p_ref_without_the_shift_is_sklearns_binary_search(n, perplexity):
    pytest.importorskip("sklearn")
    from sklearn.manifold import _utils
    X, _ = tsne_ref.clustered(n, 10, seed=n)
    ids, dist, count = tsne_ref.neighbours_l2(X, min(n - 1, int(3 * perplexity)))
    d2 = (dist.astype(np.float64) ** 2).astype(np.float32)
    want = _utils._binary_search_perplexity(np.ascontiguousarray(d2), float(perplexity), 0)
    got, _ = tsne_ref.cond_p_ref(d2.astype(np.float64), count, perplexity, tol=1e-5, shift=False)
    err = (np.abs(got - want).max(1) / want.max(1)).max()
    print("n", n, "perplexity", perplexity, "max |p - sklearn| / row max", err)
    assert err <= 1e-5
    # and the shift moves nothing where nothing underflows
    shifted, _ = tsne_ref.cond_p_ref(d2.astype(np.float64), count, perplexity, tol=1e-10)
    assert (np.abs(shifted - want).max(1) / want.max(1)).max() <= 3e-5
