"""CPU-only checks of the candidate-list ranking: kge_rank_candidates / kge_rank_lists_from_scores refuse bad arguments before any
GPU call, the header's prototypes are what _lib binds, build_type_constraints equals a brute-force dict, and Evaluator.rank_candidates /
test_candidates / test_type_constrained / test_sampled plumb lists, filters, chunks and row order correctly over an injected backend
whose two calls are the numpy restatement of the contract (tests/candidates_ref.py)."""
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


def _call(lib, desc="transe", n=4, side=0, loq=None, n_lists=4, skip_off=None, skip_ids=None, ws=FAKE, ws_bytes=1 << 20):
    d = _desc() if desc == "transe" else desc
    return lib.kge_rank_candidates(None if d is None else ctypes.byref(d), FAKE, n, side, loq, FAKE, FAKE, n_lists, skip_off, skip_ids, ws,
                                   ws_bytes, FAKE, None)


def _refusals():
    from pykg2vec_amd import _lib
    return [
        (dict(desc=None), b"null model descriptor"), (dict(side=2), b"side"), (dict(side=-1), b"side"), (dict(n=-1), b"n = -1"),
        (dict(skip_off=FAKE), b"skip_ids"), (dict(skip_ids=FAKE), b"skip_off"),
        (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace"),
        (dict(loq=FAKE, n_lists=0), b"list_of_query"), (dict(n_lists=3), b"n_lists"),
        (dict(desc=_desc(_lib.RESCAL)), b"via-forward"), (dict(desc=_desc(_lib.NTN, 6)), b"kge_rank_lists_from_scores"),
        (dict(desc=_desc(_lib.HOLE)), b"via-forward"), (dict(desc=_desc(99)), b"unknown model"), (dict(desc=_desc(tables=1)), b"table 1"),
    ]


@pytest.mark.parametrize("case", range(15))
def test_rank_candidates_refuses_bad_arguments_without_gpu(case):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    kw, word = _refusals()[case]
    assert _call(lib, **kw) != 0
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_rank_candidates_with_no_queries_is_a_no_op():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _call(lib, n=0, n_lists=0, ws=None, ws_bytes=0) == 0
    assert lib.kge_rank_lists_from_scores(FAKE, 0, FAKE, FAKE, 0, None, 0, FAKE, None) == 0


@pytest.mark.parametrize("kw, word", [(dict(dtype=2), b"dtype"), (dict(n=-1), b"n = -1"), (dict(scores=None), b"null"),
                                      (dict(counts=None), b"null")])
def test_rank_lists_from_scores_refuses_bad_arguments_without_gpu(kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    a = dict(scores=FAKE, dtype=0, n=3, counts=FAKE)
    a.update(kw)
    assert lib.kge_rank_lists_from_scores(a["scores"], a["dtype"], FAKE, FAKE, a["n"], None, 0, a["counts"], None) != 0
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_workspace_is_one_offset_per_query():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert lib.kge_rank_candidates_workspace_bytes(0, 0, 0) == 0
    for n in (1, 4096, 100000):
        need = lib.kge_rank_candidates_workspace_bytes(n, n, 64 * n)
        assert 8 * (n + 1) <= need <= 8 * (n + 1) + 1024
        assert need == lib.kge_rank_candidates_workspace_bytes(n, 3, 7)   # the lists are read in place


def test_header_prototypes_are_what_lib_binds():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_CAND_CHUNK\s+(\d+)", text).group(1)) == _lib.CAND_CHUNK == kernels.CAND_CHUNK
    assert int(re.search(r"#define\s+KGE_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 3
    ctype_of = lambda arg: (ctypes.c_void_p if "*" in arg and "kge_model_desc" not in arg else
                            ctypes.POINTER(_lib.ModelDesc) if "*" in arg else
                            {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "size_t": ctypes.c_size_t}[arg.split()[-2]])
    for name in ("kge_rank_candidates", "kge_rank_candidates_workspace_bytes", "kge_rank_lists_from_scores"):
        m = re.search(r"(\w+)\s+%s\(([^;]*)\);" % name, text)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(2).replace("\n", " ").split(",")]
        res, bound = _lib._SIGNATURES[name]
        assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)], name
        assert [ctype_of(a) for a in args] == list(bound), (name, args)
        assert name in _lib.EXPORTED_SYMBOLS


def test_type_constraints_are_the_brute_force_dicts():
    from pykg2vec_amd.evaluator import build_type_constraints
    c = Case("transe_l1")
    train = c.train[c.train[:, 1] != 1]          # relation 1 is absent from the split: an empty list on both sides
    assert (c.train[:, 1] == 1).any() and c.R > 2
    ranges, domains = build_type_constraints(train, c.R)
    tails, heads = {}, {}
    for h, r, t in train.tolist():
        tails.setdefault(r, set()).add(t)
        heads.setdefault(r, set()).add(h)
    for lists, want in ((ranges, tails), (domains, heads)):
        assert lists.n_lists == c.R and lists.list_of_query is None and lists.off.dtype == torch.int64 and lists.ids.dtype == torch.int32
        off, ids = lists.off.numpy(), lists.ids.numpy()
        for r in range(c.R):
            assert ids[off[r]:off[r + 1]].tolist() == sorted(want.get(r, ()))
        assert off[2] == off[1]
    rel = torch.tensor([2, 0, 2])
    q = ranges.for_queries(rel)
    assert torch.equal(q.off, ranges.off) and torch.equal(q.ids, ranges.ids) and q.list_of_query.tolist() == [2, 0, 2]
    empty = build_type_constraints(np.zeros((0, 3), np.int64), 4)[0]
    assert empty.n_lists == 4 and empty.ids.numel() == 0


# ---------------------------------------------------------------------------------------------- plumbing over an injected backend
class Backend(types.SimpleNamespace):
    """oracle_backend + the two candidate calls as numpy restatements, with the calls recorded."""

    def __init__(self, E):
        super().__init__(**{k: v for k, v in vars(oracle_backend).items() if not k.startswith("__")})
        self.E = E
        self.fused, self.counted = [], []

    def rank_candidates(self, desc, triples, side, cand_off, cand_ids, list_of_query=None, skip_off=None, skip_ids=None, skip_sorted=False):
        self.fused.append((side, bool(skip_sorted)))
        if skip_sorted:   # the precondition the flag promises
            o, s = skip_off.numpy(), skip_ids.numpy()
            assert all((np.diff(s[o[i]:o[i + 1]]) >= 0).all() for i in range(len(o) - 1))
        fn = lambda h, r, t: ko.score(desc.name, desc.params(), h, r, t, **desc.hp)
        return cr.rank_candidates_torch(fn, self.E, triples, side, cand_off, cand_ids, list_of_query, skip_off, skip_ids)

    def rank_lists_from_scores(self, scores, truth_scores, seg_off, flags=None, largest=False):
        self.counted.append(int(truth_scores.numel()))
        return cr.rank_lists_from_scores_torch(scores, truth_scores, seg_off, flags, largest)


def _setup(filter_source=None, via_forward=False):
    from pykg2vec_amd.evaluator import Evaluator
    c = Case("transe_l1")
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, device="cpu")
    m = hip_util.model_from_case(c, device="cpu")
    S = torch.from_numpy(np.round(np.random.default_rng(5).normal(size=997) * 2).astype(np.float32))   # quantised: ties are the rule
    if via_forward:
        m.kernel_name = "ntn"      # a model without row kernels: its own forward scores the expanded lists
        m.forward = lambda h, r, t: S[(h * 31 + r * 7 + t * 3) % 997]
    B = Backend(c.E)
    ev = Evaluator(m, cfg, backend=B)
    if filter_source:
        ev.FILTER_SOURCE = filter_source
    fn = ((lambda h, r, t: S.numpy()[(h * 31 + r * 7 + t * 3) % 997]) if via_forward else
          (lambda h, r, t: ko.score("transe", c.params(), h, r, t, **c.hp)))
    return c, cfg, m, ev, B, fn


def _lists(c, n, C, seed):
    """[n, C] tables with the true id, duplicates, -1 and ids >= E among the entries."""
    rng = np.random.default_rng(seed)
    t = rng.integers(c.E, size=(2, n, C))
    t[:, :, 0] = t[:, :, 1]                       # a duplicate
    t[0, :, 2], t[1, :, 2] = c.test[:n, 2], c.test[:n, 0]   # the true entities
    t[:, ::2, 3] = -1
    t[:, 1::2, 4] = c.E + 5
    # known entities of the pair, so that the filter has something to leave out
    hr_t, tr_h = c.filters()
    for i, (h, r, tt) in enumerate(c.test[:n].tolist()):
        for k, e in enumerate(sorted(hr_t[(h, r)])[:3]):
            t[0, i, 5 + k] = e
        for k, e in enumerate(sorted(tr_h[(tt, r)])[:3]):
            t[1, i, 5 + k] = e
    return t[0], t[1]


def _want(c, fn, q, tails, heads):
    """[4, n] + ties [2, n] in rank_all's row order, the filter from the dicts of all three splits."""
    hr_t, tr_h = c.filters()
    out = []
    for side, table in ((0, tails), (1, heads)):
        off, ids = table if isinstance(table, tuple) else cr.to_csr(table)
        known = [sorted(tr_h[(t, r)]) if side else sorted(hr_t[(h, r)]) for h, r, t in q.tolist()]
        s_off, s_ids = cr.csr_of(known)
        out.append(cr.rank_candidates_ref(fn, q, side, off, ids, c.E, None, s_off, s_ids))
    ct, ch = out
    return np.stack([ch[0], ct[0], ch[1], ct[1]]), np.stack([ch[2], ct[2]])


@pytest.mark.parametrize("source", ["dicts", "triples_host"])
def test_rank_candidates_row_order_filters_and_both_list_forms(source):
    c, cfg, m, ev, B, fn = _setup(source)
    n, C = 17, 12
    q = c.test[:n]
    tails, heads = _lists(c, n, C, 1)
    want, want_ties = _want(c, fn, q, tails, heads)
    assert (want[2] < want[0]).any() or (want[3] < want[1]).any()      # the filter matters here
    assert not np.array_equal(want[0], want[1])                        # and so does the row order
    got, ties = ev.rank_candidates(q, n, tails, torch.from_numpy(heads), return_ties=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, n) and tuple(ties.shape) == (2, n)
    assert np.array_equal(got.numpy(), want) and np.array_equal(ties.numpy(), want_ties)
    assert B.fused == [(0, source == "triples_host"), (1, source == "triples_host")] and not B.counted
    # the CSR form: ragged lists, the same entries
    from pykg2vec_amd.evaluator import CandidateLists
    ragged = [[row[:3 + i % 5].tolist() for i, row in enumerate(t)] for t in (tails, heads)]
    csr = [cr.csr_of(x) for x in ragged]
    want2, _ = _want(c, fn, q, csr[0], csr[1])
    got2 = ev.rank_candidates(q, n, CandidateLists(*csr[0]), CandidateLists(*csr[1]))
    assert np.array_equal(got2.numpy(), want2)
    # shared lists: every query mapped to one of three lists
    loq = np.arange(n) % 3
    shared = CandidateLists(*cr.csr_of(ragged[0][:3]), list_of_query=loq)
    per_query = CandidateLists(*cr.csr_of([ragged[0][k] for k in loq]))
    assert torch.equal(ev.rank_candidates(q, n, shared, shared), ev.rank_candidates(q, n, per_query, per_query))
    with pytest.raises(ValueError):
        ev.rank_candidates(q, n, tails[:5], heads)
    with pytest.raises(TypeError):
        ev.rank_candidates(q, n, tails.astype(np.float32), heads)


@pytest.mark.parametrize("source", ["dicts", "triples_host"])
def test_via_forward_chunks_cover_the_queries_and_do_not_change_the_answer(source):
    c, cfg, m, ev, B, fn = _setup(source, via_forward=True)
    n, C = 23, 12
    q = c.test[:n]
    tails, heads = _lists(c, n, C, 2)
    want, want_ties = _want(c, fn, q, tails, heads)
    assert want_ties.max() > 0
    for rows, chunks in ((1, [1] * n), (7, [7, 7, 7, 2]), (n, [n]), (1000, [n])):
        ev.PREDICT_SCRATCH_BYTES = rows * C * ev.CANDIDATE_ENTRY_BYTES
        B.counted.clear()
        got, ties = ev.rank_candidates(q, n, tails, heads, return_ties=True)
        assert B.counted == chunks * 2 and not B.fused
        assert np.array_equal(got.numpy(), want) and np.array_equal(ties.numpy(), want_ties)
    ev.PREDICT_SCRATCH_BYTES = 1   # a budget below one list still makes progress, a query at a time
    assert np.array_equal(ev.rank_candidates(q, n, tails, heads).numpy(), want)
    m.higher_is_better = True      # MuRP's direction: the counts flip to "higher is better"
    flipped, _ = _want(c, lambda h, r, t: -fn(h, r, t), q, tails, heads)
    assert np.array_equal(ev.rank_candidates(q, n, tails, heads).numpy(), flipped)


def test_test_candidates_feeds_the_metric_calculator_and_warns_about_ties(capsys):
    c, cfg, m, ev, B, fn = _setup(via_forward=True)
    n, C = 20, 12
    q = c.test[:n]
    tails, heads = _lists(c, n, C, 3)
    want, want_ties = _want(c, fn, q, tails, heads)
    got = ev.test_candidates(q, n, tails, heads, epoch=3)
    out = capsys.readouterr().out
    assert "WARNING" in out and "optimistic end" in out and "Epoch: 3" in out
    assert set(got) == {"mr", "fmr", "mrr", "fmrr"}
    for k, v in cr.metrics(want).items():
        assert got[k] == v, (k, got[k], v)
    assert np.array_equal(ev.tie_counts, want_ties)
    assert ev.metric_calculator.hit[(3, 10)] == np.mean(np.concatenate([want[0], want[1]]) + 1 <= 10, dtype=np.float32)


def test_type_constrained_and_sampled_protocols():
    from pykg2vec_amd.evaluator import build_type_constraints
    c, cfg, m, ev, B, fn = _setup()
    n = 16
    q = c.test[:n]
    ranges, domains = build_type_constraints(c.train, c.R)
    lists = [(x.off.numpy(), x.ids.numpy()) for x in (ranges, domains)]
    hr_t, tr_h = c.filters()
    per_side = []
    for side in (0, 1):
        known = [sorted(tr_h[(t, r)]) if side else sorted(hr_t[(h, r)]) for h, r, t in q.tolist()]
        per_side.append(cr.rank_candidates_ref(fn, q, side, lists[side][0], lists[side][1], c.E, q[:, 1], *cr.csr_of(known)))
    ct, ch = per_side
    want = cr.metrics(np.stack([ch[0], ct[0], ch[1], ct[1]]))
    got = ev.test_type_constrained(q, n)
    assert all(got[k] == want[k] for k in want), (got, want)
    assert ev.test_type_constrained(n=n) == got            # data defaults to the test split
    # sampled: the same seed draws the same candidates, another seed other ones; the lists have num_candidates entries
    a, b, other = ev.test_sampled(q, n, 9, seed=4), ev.test_sampled(q, n, 9, seed=4), ev.test_sampled(q, n, 9, seed=5)
    assert a == b and a != other
    assert a["mr"] <= 10 and "num_candidates + 1" in type(ev).test_sampled.__doc__


def test_projection_models_are_refused():
    c, cfg, m, ev, B, fn = _setup()
    from pykg2vec_amd.projection import TuckER
    ev.model = TuckER(tot_entity=c.E, tot_relation=c.R, ent_hidden_size=8, rel_hidden_size=4, lmbda=0.0, input_dropout=0.3, hidden_dropout1=0.4,
                      hidden_dropout2=0.5)
    with pytest.raises(ValueError, match="projection"):
        ev.rank_candidates(c.test[:4], 4, np.zeros((4, 2), np.int64), np.zeros((4, 2), np.int64))
    with pytest.raises(ValueError, match="rank_all"):
        ev.test_sampled(c.test[:4], 4, 3)
