"""CPU-only checks of the nearest-neighbour search: header, ctypes binding and exported symbols agree; kge_knn_rows refuses bad
arguments before any GPU call; Model.entity_matrix / relation_matrix take the expected tables for every golden case; and
Evaluator.nearest_* / find_duplicates / Trainer.infer_similar_* plumb queries, chunks, self-exclusion and names correctly over an injected
backend whose search is the numpy restatement of the contract (tests/knn_ref.py)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import hip_util
import knn_ref
import oracle_backend
from golden_util import CASES, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _call(lib, n_rows=100, dim=8, tstride=8, nq=4, qstride=8, k=5, metric=1, table=FAKE, queries=FAKE, ws=FAKE, ws_bytes=1 << 30,
          out_ids=FAKE, out_scores=FAKE, out_count=FAKE):
    return lib.kge_knn_rows(table, n_rows, dim, tstride, queries, nq, qstride, None, k, metric, ws, ws_bytes, out_ids, out_scores, out_count, None)


@pytest.mark.parametrize("kw, word", [
    (dict(k=0), b"k = 0"), (dict(k=129), b"k = 129"), (dict(dim=0, tstride=0, qstride=0), b"dim"), (dict(metric=3), b"metric"),
    (dict(metric=-1), b"metric"), (dict(n_rows=0), b"n_rows"), (dict(tstride=7), b"table_stride"), (dict(qstride=7), b"query_stride"),
    (dict(table=None), b"null"), (dict(queries=None), b"null"), (dict(out_ids=None), b"null"), (dict(out_scores=None), b"null"),
    (dict(out_count=None), b"null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace"),
])
def test_knn_rows_refuses_bad_arguments_without_gpu(kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) == -1
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_knn_workspace_holds_the_partial_lists_and_the_norms(monkeypatch):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    monkeypatch.delenv("KGE_KNN_SPLIT", raising=False)
    for nq, n_rows, k in ((1, 123182, 10), (1024, 14951, 10), (14951, 14951, 100), (5, 3, 128)):
        dot = lib.kge_knn_workspace_bytes(nq, n_rows, 100, k, 0)
        l2 = lib.kge_knn_workspace_bytes(nq, n_rows, 100, k, 2)
        assert nq * k * 8 <= dot <= nq * (2048 * 8) + 1024          # S * k pairs per query, S * k <= 2048
        assert dot + 4 * (nq + n_rows) <= l2 <= dot + 4 * (nq + n_rows) + 1024
    # one query over 123 k candidates is not one workgroup's job: the lists of many slabs
    assert lib.kge_knn_workspace_bytes(1, 123182, 100, 10, 0) >= 32 * 10 * 8
    monkeypatch.setenv("KGE_KNN_SPLIT", "1")
    assert lib.kge_knn_workspace_bytes(1, 123182, 100, 10, 0) <= 10 * 8 + 1024
    assert lib.kge_knn_workspace_bytes(4, 100, 8, 0, 0) == 0      # refused arguments ask for nothing


def test_knn_header_binding_and_constants_agree():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_KNN_MAX\s+(\d+)", text).group(1)) == _lib.KNN_MAX == kernels.KNN_MAX == 128
    for name, code in _lib.KNN_METRICS.items():
        assert int(re.search(r"#define\s+KGE_KNN_%s\s+(\d+)" % name.upper(), text).group(1)) == code
    lib = _lib.load()
    for sym in ("kge_knn_workspace_bytes", "kge_knn_rows"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        proto = re.search(r"\b%s\(([^;]*)\);" % sym, text).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[sym][1]), sym
    assert _lib.ABI_VERSION == 3   # additive entry points


def test_knn_rows_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from pykg2vec_amd import _lib, kernels
    t, q = torch.zeros(10, 4), torch.zeros(3, 4)
    with pytest.raises(_lib.KgeHipError):
        kernels.knn_rows(t, q, 3)
    with pytest.raises(TypeError):
        kernels.knn_rows(t.double(), q, 3)
    with pytest.raises(TypeError):
        kernels.knn_rows(t[0], q, 3)
    with pytest.raises(ValueError):
        kernels.knn_metric("manhattan")


# ------------------------------------------------------------------------------------------------------- which tables are searched
E_ONLY, R_ONLY = ("ent_embedding",), ("rel_embedding",)
EXPECTED = {
    "transe": (E_ONLY, R_ONLY), "transm": (E_ONLY, R_ONLY), "distmult": (E_ONLY, R_ONLY), "ntn": (E_ONLY, R_ONLY),
    "transh": (E_ONLY, ("rel_embedding", "w")),
    "transd": (("ent_embedding", "ent_mappings"), ("rel_embedding", "rel_mappings")),
    "rotate": (("ent_embeddings_real", "ent_embeddings_imag"), ("rel_embeddings_real",)),
    "rescal": (E_ONLY, ("rel_matrices",)),
    "transr": (E_ONLY, ("rel_embedding", "rel_matrix")),
    "complex": (("emb_e_real", "emb_e_img"), ("emb_rel_real", "emb_rel_img")),
    "complexn3": (("emb_e_real", "emb_e_img"), ("emb_rel_real", "emb_rel_img")),
    "analogy": (("ent_embedding", "emb_e_real", "emb_e_img"), ("rel_embedding", "emb_rel_real", "emb_rel_img")),
    "cp": (("sub_embedding", "obj_embedding"), R_ONLY),
    "simple": (("ent_head_embedding", "ent_tail_embedding"), ("rel_embedding", "rel_inv_embedding")),
    "simple_ignr": (("ent_head_embedding", "ent_tail_embedding"), ("rel_embedding", "rel_inv_embedding")),
    # (the four rel_{s,x,y,z} tables carry tot_entity rows, as the reference's do: the relations' own rows are taken)
    "quate": (tuple("ent_%s_embedding" % c for c in "sxyz"), tuple("rel_%s_embedding" % c for c in "sxyzw")),
}


@pytest.mark.parametrize("name", CASES)
def test_entity_and_relation_matrix_take_the_expected_tables(name):
    c = Case(name)
    m = hip_util.model_from_case(c, device="cpu")
    by_name = {p.name: p.weight.detach() for p in m.parameter_list}
    for kind, names, rows in (("entity", EXPECTED[c.model][0], c.E), ("relation", EXPECTED[c.model][1], c.R)):
        got = m.entity_matrix() if kind == "entity" else m.relation_matrix()
        want = torch.cat([by_name[n][:rows].float() for n in names], 1)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and got.shape[0] == rows
        assert torch.equal(got, want), (name, kind)
        if len(names) == 1 and by_name[names[0]].shape[0] == rows:
            assert got.data_ptr() == by_name[names[0]].data_ptr()      # one table: passed as it is, no copy
    one = m.entity_matrix(tables=EXPECTED[c.model][0][-1:])
    assert torch.equal(one, by_name[EXPECTED[c.model][0][-1]][:c.E].float())
    with pytest.raises(KeyError):
        m.entity_matrix(tables=["no_such_table"])


def test_matrix_of_float64_tables_is_converted():
    c = Case("transe_l1")
    m = hip_util.model_from_case(c, device="cpu")
    m.ent_embeddings.weight.data = m.ent_embeddings.weight.data.double()
    got = m.entity_matrix()
    assert got.dtype == torch.float32 and torch.equal(got, m.ent_embeddings.weight.detach().float())


# ---------------------------------------------------------------------------------------------- plumbing over an injected backend
class Backend(types.SimpleNamespace):
    """oracle_backend (what Trainer.build_model needs on the CPU) + the numpy search, with the calls recorded."""

    def __init__(self):
        super().__init__(**{k: v for k, v in vars(oracle_backend).items() if not k.startswith("__")})
        self.chunks = []

    def knn_rows(self, table, queries, k, metric="cosine", self_ids=None):
        self.chunks.append((int(queries.shape[0]), self_ids is not None))
        return knn_ref.knn_rows_torch(table, queries, k, metric, self_ids)


def _setup(case="transe_l1"):
    c = Case(case)
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, device="cpu")
    cfg.knowledge_graph.cache.update(idx2entity={i: "e%d" % i for i in range(c.E)}, idx2relation={i: "r%d" % i for i in range(c.R)})
    m = hip_util.model_from_case(c, device="cpu")
    from pykg2vec_amd.evaluator import Evaluator
    B = Backend()
    return c, cfg, m, Evaluator(m, cfg, backend=B), B


def _quantise(m):
    """Entity rows on a coarse grid, so that tie groups are the rule."""
    w = m.ent_embeddings.weight.data
    w.copy_(torch.round(w * 8 / w.abs().max()))
    return w.numpy()


def test_nearest_chunks_cover_the_queries_and_do_not_change_the_answer():
    c, cfg, m, ev, B = _setup()
    W = _quantise(m)
    ids = np.random.default_rng(0).integers(c.E, size=23)
    for metric in knn_ref.METRICS:
        want = knn_ref.knn_ref(W, W[ids], 7, metric, ids)
        for rows, chunks in ((1, [1] * 23), (7, [7, 7, 7, 2]), (23, [23]), (1000, [23])):
            ev.PREDICT_SCRATCH_BYTES = rows * ev.KNN_QUERY_BYTES + 4 * c.E
            B.chunks.clear()
            got, vals = ev.nearest_entities(ids.tolist() if rows == 7 else torch.from_numpy(ids), topk=7, metric=metric)
            assert B.chunks == [(n, True) for n in chunks]
            assert got.dtype == torch.int64 and tuple(got.shape) == (23, 7) and vals.dtype == torch.float32
            assert np.array_equal(got.numpy(), want[0]) and np.array_equal(vals.numpy(), want[1].astype(np.float32))
    ev.PREDICT_SCRATCH_BYTES = 1      # a budget below one query still makes progress, a query at a time
    B.chunks.clear()
    got, _ = ev.nearest_entities(ids[:3], topk=2, metric="l2", exclude_self=False)
    assert B.chunks == [(1, False)] * 3
    assert np.array_equal(got.numpy(), knn_ref.knn_ref(W, W[ids[:3]], 2, "l2")[0])     # the row itself is a candidate now
    for bad in (0, 129):
        with pytest.raises(ValueError, match="KGE_KNN_MAX"):
            ev.nearest_entities([0], topk=bad)
    with pytest.raises(ValueError, match="metric"):
        ev.nearest_entities([0], metric="l1")


def test_nearest_relations_and_vectors_search_the_right_matrix():
    c, cfg, m, ev, B = _setup("transh_l1")
    Rm = m.relation_matrix().numpy()             # [rel_embedding | w]
    k = min(c.R - 1, 4)
    got, _ = ev.nearest_relations([1, 0], topk=k, metric="dot")
    assert np.array_equal(got.numpy(), knn_ref.knn_ref(Rm, Rm[[1, 0]], k, "dot", [1, 0])[0])
    got, _ = ev.nearest_relations([1], topk=k, metric="dot", tables=["w"])
    Wn = m.w.weight.detach().numpy()
    assert np.array_equal(got.numpy(), knn_ref.knn_ref(Wn, Wn[[1]], k, "dot", [1])[0])
    Em = m.entity_matrix().numpy()
    v = (Em[[3, 5]] + m.rel_embeddings.weight.detach().numpy()[[1, 2]]).astype(np.float32)
    B.chunks.clear()
    got, vals = ev.nearest_to_vectors(v, kind="entity", topk=5, metric="l2")
    assert B.chunks == [(2, False)]
    want = knn_ref.knn_ref(Em, v, 5, "l2")
    assert np.array_equal(got.numpy(), want[0]) and np.array_equal(vals.numpy(), want[1].astype(np.float32))
    assert tuple(ev.nearest_to_vectors(v[0], topk=3)[0].shape) == (1, 3)       # one vector: one query
    with pytest.raises(ValueError):
        ev.nearest_to_vectors(v[:, :3])
    with pytest.raises(ValueError):
        ev.nearest_to_vectors(v, kind="triple")


def test_find_duplicates_lists_every_pair_once_in_order():
    c, cfg, m, ev, B = _setup()
    w = m.ent_embeddings.weight.data
    group, pair = [2, 11, 7], [5, 9]                  # three copies and two copies
    for g in (group, pair):
        for e in g[1:]:
            w[e] = w[g[0]]
    ev.PREDICT_SCRATCH_BYTES = 10 * ev.KNN_QUERY_BYTES + 4 * c.E
    pairs, scores = ev.find_duplicates(kind="entity", metric="l2", threshold=0.0, topk=4)
    assert pairs.dtype == torch.int64 and pairs.shape[1] == 2
    assert pairs.tolist() == [[2, 7], [2, 11], [5, 9], [7, 11]] and scores.tolist() == [0.0] * 4
    assert sum(n for n, _ in B.chunks) == c.E and all(s for _, s in B.chunks) and max(n for n, _ in B.chunks) == 10
    # a similarity threshold passes from above; every pair (a < b) once although both a's and b's rows list it
    W = w.numpy()
    S = knn_ref.scores64(W, W, "cosine").astype(np.float32)
    thr = float(np.sort(S[np.triu_indices(c.E, 1)])[-12])
    pairs, scores = ev.find_duplicates(metric="cosine", threshold=thr, topk=c.E - 1 if c.E - 1 <= 128 else 128)
    got = pairs.tolist()
    assert got and got == [list(p) for p in sorted(set(map(tuple, got)))] and all(a < b for a, b in got)
    if c.E - 1 <= 128:
        a, b = np.nonzero(np.triu(S >= thr, 1))
        assert got == list(map(list, zip(a.tolist(), b.tolist())))
        assert np.array_equal(scores.numpy(), S[a, b])
    with pytest.raises(ValueError, match="threshold"):
        ev.find_duplicates()


def test_trainer_infer_similar_returns_names_nearest_first():
    from pykg2vec_amd.trainer import Trainer
    c, cfg, m, ev, B = _setup()
    tr = Trainer(m, cfg, backend=B)
    tr.build_model()
    W = tr.model.entity_matrix().numpy()
    got = tr.infer_similar_entities(4, topk=5)
    want = knn_ref.knn_ref(W, W[[4]], 5, "cosine", [4])[0][0].tolist()
    assert 4 not in got and list(got) == want and got == {e: "e%d" % e for e in want}
    Rm = tr.model.relation_matrix().numpy()
    got = tr.infer_similar_relations(1, topk=c.R + 3, metric="l2")        # more places than live relations: padding dropped
    want = [i for i in knn_ref.knn_ref(Rm, Rm[[1]], min(c.R + 3, 128), "l2", [1])[0][0].tolist() if i >= 0]
    assert list(got) == want and len(got) == c.R - 1 and got == {i: "r%d" % i for i in want}
