"""CPU-only checks of the relation ranking: kge_rank_relations / kge_relation_csr_* refuse bad arguments before any GPU call, the
header's prototypes are what _lib binds, build_relation_csr_from_triples equals a brute-force dict, and Evaluator.rank_relations /
test_relations plumb filters, chunks, caching and metrics correctly over an injected backend whose calls are the numpy restatement
of the contract (tests/relations_ref.py)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import candidates_ref as cr
import hip_util
import kge_oracle as ko
import oracle_backend
import relations_ref as rr
from golden_util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _desc(model=None, tables=2):
    from pykg2vec_amd import _lib
    d = _lib.ModelDesc()
    d.model = _lib.TRANSE if model is None else model
    d.tot_entity, d.tot_relation, d.dim, d.rel_dim = 50, 5, 20, 20
    for i in range(tables):
        d.tables[i] = 256
    return d


def _call(lib, desc="transe", triples=FAKE, n=4, skip_off=None, skip_ids=None, ws=FAKE, ws_bytes=1 << 20, counts=FAKE):
    d = _desc() if desc == "transe" else desc
    return lib.kge_rank_relations(None if d is None else ctypes.byref(d), triples, n, skip_off, skip_ids, ws, ws_bytes, counts, None)


def _refusals():
    from pykg2vec_amd import _lib
    return [
        (dict(desc=None), b"null model descriptor"), (dict(n=-1), b"n = -1"),
        (dict(skip_off=FAKE), b"skip_ids"), (dict(skip_ids=FAKE), b"skip_off"),
        (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace"),
        (dict(triples=None), b"triples"), (dict(counts=None), b"counts"),
        (dict(desc=_desc(tables=1)), b"table 1"),
        (dict(desc=_desc(_lib.RESCAL)), b"via-forward"), (dict(desc=_desc(_lib.NTN, 6)), b"kge_rank_lists_from_scores"),
        (dict(desc=_desc(_lib.HOLE)), b"via-forward"), (dict(desc=_desc(99)), b"unknown model"),
    ]


@pytest.mark.parametrize("case", range(13))
def test_rank_relations_refuses_bad_arguments_without_gpu(case):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    kw, word = _refusals()[case]
    assert _call(lib, **kw) != 0
    assert word in lib.kge_last_error() and b"kge_rank_relations" in lib.kge_last_error(), lib.kge_last_error()


def test_rank_relations_with_no_queries_is_a_no_op():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert lib.kge_rank_relations_workspace_bytes(0) == 0
    assert _call(lib, n=0, ws=None, ws_bytes=0, triples=None, counts=None) == 0
    need = lib.kge_rank_relations_workspace_bytes(1)
    assert 0 < need <= 1024 and need == lib.kge_rank_relations_workspace_bytes(1 << 20)    # the arguments' copy: no per-query state


def _csr_count(lib, known=FAKE, n_known=10, queries=FAKE, n=4, E=50, R=5, ws=FAKE, ws_bytes=1 << 20, off=FAKE, total=FAKE):
    return lib.kge_relation_csr_count(known, n_known, queries, n, E, R, ws, ws_bytes, off, total, None)


@pytest.mark.parametrize("kw, word", [
    (dict(E=(1 << 24) + 1), b"2^24"), (dict(R=(1 << 16) + 1), b"2^16"), (dict(known=None), b"known"), (dict(queries=None), b"queries"),
    (dict(ws=None), b"workspace"), (dict(off=None), b"rel_off"), (dict(total=None), b"total"), (dict(n_known=0), b"n_known"),
    (dict(n=0), b"n_queries"), (dict(ws_bytes=64), b"workspace too small")])
def test_relation_csr_refuses_bad_arguments_without_gpu(kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _csr_count(lib, **kw) != 0
    assert word in lib.kge_last_error() and b"kge_relation_csr_count" in lib.kge_last_error(), lib.kge_last_error()
    assert lib.kge_relation_csr_fill(FAKE, 4, 10, FAKE, FAKE, None, None) != 0
    assert b"kge_relation_csr_fill" in lib.kge_last_error()


def test_relation_csr_workspace_holds_one_key_per_known_triple():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert lib.kge_relation_csr_workspace_bytes(0, 4) == 0
    for M, P in ((1, 2048), (2048, 2048), (2049, 4096), (100000, 131072)):
        need = lib.kge_relation_csr_workspace_bytes(M, 100)
        assert 8 * P + 4 * 101 <= need <= 8 * P + 4 * 101 + 1024
        assert need < lib.kge_filter_csr_workspace_bytes(M, 100)      # one side, not two


def test_header_prototypes_are_what_lib_binds():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_REL_CHUNK\s+(\d+)", text).group(1)) == _lib.REL_CHUNK == kernels.REL_CHUNK
    assert int(re.search(r"#define\s+KGE_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 3
    ctype_of = lambda arg: (ctypes.c_void_p if "*" in arg and "kge_model_desc" not in arg else
                            ctypes.POINTER(_lib.ModelDesc) if "*" in arg else
                            {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "size_t": ctypes.c_size_t}[arg.split()[-2]])
    for name in ("kge_rank_relations", "kge_rank_relations_workspace_bytes", "kge_relation_csr_workspace_bytes", "kge_relation_csr_count",
                 "kge_relation_csr_fill"):
        m = re.search(r"(\w+)\s+%s\(([^;]*)\);" % name, text)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(2).replace("\n", " ").split(",")]
        res, bound = _lib._SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)], name
        assert [ctype_of(a) for a in args] == list(bound), (name, args)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)


def test_numpy_relation_csr_is_the_brute_force_dict():
    from pykg2vec_amd.evaluator import build_relation_csr_from_triples
    c = Case("transe_l1")
    known = np.concatenate([c.train, c.valid, c.test, c.train[:40]])          # duplicates across "splits"
    extra = c.test[:6].copy()
    extra[:, 1] = (extra[:, 1] + 1) % c.R                                     # pairs that carry more than one relation
    known = np.concatenate([known, extra])
    q = np.concatenate([c.test[:30], [[c.E - 1, 0, c.E - 1], [0, 1, c.E - 1]]])
    want = rr.known_relations(known, q)
    assert any(len(x) > 1 for x in want) and any(len(x) == 0 for x in want)   # several relations for a pair, and an absent pair
    off, ids = build_relation_csr_from_triples(q, known, c.E)
    assert off.dtype == np.int64 and ids.dtype == np.int32 and len(off) == len(q) + 1
    assert [ids[off[i]:off[i + 1]].tolist() for i in range(len(q))] == want
    # the key is the PAIR: (h, t) and (t, h) are different pairs
    off2, ids2 = build_relation_csr_from_triples([[3, 0, 5], [5, 0, 3]], [[3, 2, 5], [3, 1, 5], [3, 2, 5]], 7)
    assert off2.tolist() == [0, 2, 2] and ids2.tolist() == [1, 2]
    off3, ids3 = build_relation_csr_from_triples(q, np.zeros((0, 3), np.int64), c.E)
    assert off3.tolist() == [0] * (len(q) + 1) and ids3.dtype == np.int32 and ids3.size == 0
    off4, ids4 = build_relation_csr_from_triples(np.zeros((0, 3), np.int64), known, c.E)
    assert off4.tolist() == [0] and ids4.size == 0


# ---------------------------------------------------------------------------------------------- plumbing over an injected backend
class Backend(types.SimpleNamespace):
    """oracle_backend + the relation calls as numpy restatements, with the calls recorded."""

    def __init__(self, R):
        super().__init__(**{k: v for k, v in vars(oracle_backend).items() if not k.startswith("__")})
        self.R = R
        self.fused, self.counted = [], []

    def rank_relations(self, desc, triples, skip_off=None, skip_ids=None, skip_sorted=False):
        self.fused.append((int(triples.shape[0]), bool(skip_sorted)))
        if skip_sorted:   # the precondition the flag promises
            o, s = skip_off.numpy(), skip_ids.numpy()
            assert all((np.diff(s[o[i]:o[i + 1]]) > 0).all() for i in range(len(o) - 1))
        fn = lambda h, r, t: ko.score(desc.name, desc.params(), h, r, t, **desc.hp)
        return rr.rank_relations_torch(fn, self.R, triples, skip_off, skip_ids)

    def rank_lists_from_scores(self, scores, truth_scores, seg_off, flags=None, largest=False):
        self.counted.append(int(truth_scores.numel()))
        return cr.rank_lists_from_scores_torch(scores, truth_scores, seg_off, flags, largest)


def _setup(via_forward=False):
    from pykg2vec_amd.evaluator import Evaluator
    c = Case("transe_l1")
    extra = c.test[:12].copy()
    extra[:, 1] = (extra[:, 1] + 1 + np.arange(12) % 2) % c.R           # other relations known for the test pairs: the filter matters
    train = np.concatenate([c.train, extra])
    cfg = hip_util.make_config(c.E, c.R, c.hp, train, c.valid, c.test, device="cpu")
    m = hip_util.model_from_case(c, device="cpu")
    S = torch.from_numpy(np.round(np.random.default_rng(5).normal(size=997) * 2).astype(np.float32))   # quantised: ties are the rule
    if via_forward:
        m.kernel_name = "ntn"      # a model without row kernels: its own forward scores the expanded triples
        m.forward = lambda h, r, t: S[(h * 31 + r * 7 + t * 3) % 997]
    B = Backend(c.R)
    ev = Evaluator(m, cfg, backend=B)
    fn = ((lambda h, r, t: S.numpy()[(h * 31 + r * 7 + t * 3) % 997]) if via_forward else
          (lambda h, r, t: ko.score("transe", c.params(), h, r, t, **c.hp)))
    known = np.concatenate([train, c.valid, c.test])
    return c, cfg, m, ev, B, fn, known


def _want(c, fn, q, known, largest=False):
    counts = rr.rank_relations_ref(fn, q, c.R, *rr.csr_of(rr.known_relations(known, q)), largest=largest)
    return counts[:2], counts[2]


def test_rank_relations_rows_filter_and_caching_by_content():
    c, cfg, m, ev, B, fn, known = _setup()
    assert c.R > 2
    n = 17
    q = c.test[:n]
    want, want_ties = _want(c, fn, q, known)
    assert (want[1] < want[0]).any()                      # the filter left something out
    got, ties = ev.rank_relations(q, n, return_ties=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, n) and ties.dtype == torch.int32 and tuple(ties.shape) == (n,)
    assert np.array_equal(got.numpy(), want) and np.array_equal(ties.numpy(), want_ties)
    assert B.fused == [(n, True)] and not B.counted
    assert tuple(ev.rank_relations(q, n).shape) == (2, n)
    # cached by content: an equal array is a hit, a different one of the same shape is not; n cuts the data
    calls = []
    real = ev._relation_csr
    ev._relation_csr = lambda trip, dev: calls.append(len(trip)) or real(trip, dev)
    ev.rank_relations(q.copy(), n)
    assert calls == []
    other = c.test[5:5 + n].copy()
    got2 = ev.rank_relations(other, n)
    assert calls == [n] and np.array_equal(got2.numpy(), _want(c, fn, other, known)[0])
    got3 = ev.rank_relations(c.test, 5)
    assert calls == [n, 5] and np.array_equal(got3.numpy(), want[:, :5])
    objs = [types.SimpleNamespace(h=int(h), r=int(r), t=int(t)) for h, r, t in q]      # Triple objects, as the reference caches them
    assert np.array_equal(ev.rank_relations(objs, n).numpy(), want)


def test_via_forward_chunks_cover_the_queries_and_do_not_change_the_answer():
    c, cfg, m, ev, B, fn, known = _setup(via_forward=True)
    n = 23
    q = c.test[:n]
    want, want_ties = _want(c, fn, q, known)
    assert want_ties.max() > 0 and (want[1] < want[0]).any()
    for rows, chunks in ((1, [1] * n), (7, [7, 7, 7, 2]), (n, [n]), (1000, [n])):
        ev.PREDICT_SCRATCH_BYTES = rows * (c.R - 1) * ev.CANDIDATE_ENTRY_BYTES
        B.counted.clear()
        got, ties = ev.rank_relations(q, n, return_ties=True)
        assert B.counted == chunks and not B.fused
        assert np.array_equal(got.numpy(), want) and np.array_equal(ties.numpy(), want_ties)
    ev.PREDICT_SCRATCH_BYTES = 1   # a budget below one query still makes progress, a query at a time
    assert np.array_equal(ev.rank_relations(q, n).numpy(), want)
    m.higher_is_better = True      # MuRP's direction: the counts flip to "higher is better"
    flipped, _ = _want(c, fn, q, known, largest=True)
    assert np.array_equal(ev.rank_relations(q, n).numpy(), flipped) and not np.array_equal(flipped, want)


def test_test_relations_metric_arithmetic_and_tie_warning(capsys):
    c, cfg, m, ev, B, fn, known = _setup(via_forward=True)
    n = 20
    want, want_ties = _want(c, fn, c.test[:n], known)
    got = ev.test_relations(c.test[:n], n, epoch=3)
    out = capsys.readouterr().out
    assert "WARNING" in out and "optimistic end" in out and "true relation's" in out and "Epoch: 3" in out
    assert set(got) == {"mr", "fmr", "mrr", "fmrr", "hits", "fhits"} and sorted(got["hits"]) == sorted(cfg.hits) == sorted(got["fhits"])
    assert rr.same_metrics(got, rr.metrics(want, cfg.hits)), (got, rr.metrics(want, cfg.hits))
    assert got["mr"].dtype == np.float32 and got["hits"][1].dtype == np.float32
    assert got["hits"][3] == np.float32((want[0] + 1 <= 3).sum()) / np.float32(n)
    assert np.array_equal(ev.relation_tie_counts, want_ties)
    assert ev.tie_counts is None                         # the entity side's record is not touched
    full = ev.test_relations()                           # data defaults to the test split, n to all of it
    assert rr.same_metrics(full, rr.metrics(_want(c, fn, c.test, known)[0], cfg.hits))


def test_projection_and_unknown_models_are_refused():
    c, cfg, m, ev, B, fn, known = _setup()
    from pykg2vec_amd.projection import TuckER
    ev.model = TuckER(tot_entity=c.E, tot_relation=c.R, ent_hidden_size=8, rel_hidden_size=4, lmbda=0.0, input_dropout=0.3, hidden_dropout1=0.4,
                      hidden_dropout2=0.5)
    with pytest.raises(ValueError, match="projection"):
        ev.rank_relations(c.test[:4], 4)
    with pytest.raises(ValueError, match="projection"):
        ev.test_relations(c.test[:4], 4)
    ev.model = m
    m.kernel_name = "no_such_model"
    with pytest.raises(ValueError, match="no relation-ranking path"):
        ev.rank_relations(c.test[:4], 4)
