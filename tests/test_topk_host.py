"""CPU-only checks of the batched link prediction: kge_topk_rows refuses bad arguments before any GPU call, the header's limit is
the Python constant, and Evaluator.predict_* / Trainer.infer_* plumb queries, chunks, filters and names correctly over an injected
backend whose select is the numpy restatement of the contract (tests/topk_ref.py) and a model whose score_rows is a fixed table."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import hip_util
import oracle_backend
import topk_ref
from golden_util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(lib, dtype=0, nq=4, n_cand=100, row_stride=100, k=5, skip_off=None, skip_ids=None, ws=None, ws_bytes=0):
    fake = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call
    return lib.kge_topk_rows(fake, dtype, nq, n_cand, row_stride, k, 0, skip_off, skip_ids, None, ws, ws_bytes, fake, fake, fake, None)


@pytest.mark.parametrize("kw, word", [
    (dict(k=0), b"k = 0"), (dict(k=1025), b"k = 1025"), (dict(dtype=2), b"dtype"), (dict(row_stride=99), b"row_stride"),
    (dict(n_cand=0, row_stride=0), b"n_cand"), (dict(skip_off=ctypes.c_void_p(256)), b"skip_ids"),
    (dict(skip_off=ctypes.c_void_p(256), skip_ids=ctypes.c_void_p(256)), b"workspace"),
    (dict(skip_off=ctypes.c_void_p(256), skip_ids=ctypes.c_void_p(256), ws=ctypes.c_void_p(256), ws_bytes=16), b"workspace"),
])
def test_topk_rows_refuses_bad_arguments_without_gpu(kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) != 0
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_topk_workspace_is_a_bit_per_candidate_and_empty_without_a_mask():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert lib.kge_topk_workspace_bytes(1000, 14951, 0) == 0
    need = lib.kge_topk_workspace_bytes(1000, 14951, 1)
    assert 1000 * 468 * 4 <= need <= 1000 * 468 * 4 + 1024


def test_topk_limit_in_header_is_the_python_constant():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_TOPK_MAX\s+(\d+)", text).group(1)) == _lib.TOPK_MAX == kernels.TOPK_MAX == 1024
    assert _lib.ABI_VERSION == 3


# ---------------------------------------------------------------------------------------------- plumbing over an injected backend
class Backend(types.SimpleNamespace):
    """oracle_backend (what Trainer.build_model needs on the CPU) + the numpy select, with the calls recorded."""

    def __init__(self):
        super().__init__(**{k: v for k, v in vars(oracle_backend).items() if not k.startswith("__")})
        self.chunks = []

    def topk_rows(self, scores, k, largest=False, skip_off=None, skip_ids=None, keep=None):
        self.chunks.append(int(scores.shape[0]))
        return topk_ref.topk_rows_torch(scores, k, largest, skip_off, skip_ids, keep)


def _table(E, rows=11, seed=3):
    """Fixed score rows, quantised so that tie groups are the rule."""
    return np.round(np.random.default_rng(seed).normal(size=(rows, E)) * 2).astype(np.float32)


def _setup(filter_source=None, names=True):
    c = Case("transe_l1")
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test, device="cpu")
    if names:
        cfg.knowledge_graph.cache.update(idx2entity={i: "e%d" % i for i in range(c.E)}, idx2relation={i: "r%d" % i for i in range(c.R)})
    m = hip_util.model_from_case(c, device="cpu")
    S = _table(c.E)
    row_of = lambda q, side: (q[:, 2 if side else 0] * 5 + q[:, 1] * 3 + side) % S.shape[0]
    m.score_rows = lambda queries, side: torch.from_numpy(S[row_of(queries.numpy(), side)])
    from pykg2vec_amd.evaluator import Evaluator
    B = Backend()
    ev = Evaluator(m, cfg, backend=B)
    if filter_source:
        ev.FILTER_SOURCE = filter_source
    return c, cfg, m, ev, B, S, row_of


def test_predict_chunks_cover_the_queries_and_do_not_change_the_answer():
    c, cfg, m, ev, B, S, row_of = _setup()
    rng = np.random.default_rng(0)
    n = 23
    h, r = rng.integers(c.E, size=n), rng.integers(c.R, size=n)
    q = np.stack([h, r, np.zeros(n, np.int64)], 1)
    want = topk_ref.topk_ref(S[row_of(q, 0)], 7)
    for rows, chunks in ((1, [1] * 23), (7, [7, 7, 7, 2]), (23, [23]), (1000, [23])):
        ev.PREDICT_SCRATCH_BYTES = rows * c.E * ev.PREDICT_ROW_ITEM_BYTES
        B.chunks.clear()
        ids, vals = ev.predict_tails(h.tolist() if rows == 7 else torch.from_numpy(h), r, topk=7)
        assert B.chunks == chunks
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (n, 7) and vals.dtype == torch.float32
        assert np.array_equal(ids.numpy(), want[0]) and np.array_equal(vals.numpy(), want[1])
    ev.PREDICT_SCRATCH_BYTES = 1   # a budget below one row still makes progress, a row at a time
    B.chunks.clear()
    assert np.array_equal(ev.predict_heads(r, h, topk=3)[0].numpy(), topk_ref.topk_ref(S[row_of(q[:, ::-1], 1)], 3)[0])
    assert B.chunks == [1] * n
    one = ev.predict_tails(int(h[0]), int(r[0]), topk=4)   # plain ints: one query
    assert np.array_equal(one[0].numpy(), want[0][:1, :4])
    with pytest.raises(ValueError):
        ev.predict_tails([1, 2], [1], topk=3)


@pytest.mark.parametrize("source", ["dicts", "triples_host"])
def test_predict_filtered_leaves_known_entities_out_and_pads(source):
    c, cfg, m, ev, B, S, row_of = _setup(source)
    hr_t, tr_h = c.filters()
    trip = c.test[:16]
    absent = np.asarray([[0, c.R - 1, 0]])     # a pair the dicts may not hold: an empty list, not a KeyError
    trip = np.concatenate([trip, absent])
    ev.PREDICT_SCRATCH_BYTES = 5 * c.E * ev.PREDICT_ROW_ITEM_BYTES
    k = c.E    # every live candidate: the rows are padded by as many places as the filter removed
    assert k <= 1024
    for side, (ea, eb), known_of in ((0, (0, 2), lambda h, r, t: hr_t.get((h, r), set())), (1, (2, 0), lambda h, r, t: tr_h.get((t, r), set()))):
        fn = (lambda **kw: ev.predict_heads(trip[:, 1], trip[:, 2], **kw)) if side else (lambda **kw: ev.predict_tails(trip[:, 0], trip[:, 1], **kw))
        ids, vals = (x.numpy() for x in fn(topk=k, filtered=True))
        kept, _ = (x.numpy() for x in fn(topk=k, filtered=True, keep=trip[:, eb].tolist()))
        for i, (h, r, t) in enumerate(trip.tolist()):
            known = known_of(h, r, t)
            live = ids[i][ids[i] >= 0]
            assert not set(live.tolist()) & known
            assert len(live) == c.E - len(known) and (ids[i][len(live):] == -1).all() and np.isnan(vals[i][len(live):]).all()
            true = (h, r, t)[eb]
            row = S[row_of(trip[i:i + 1], side)][0]
            order = topk_ref.row_order(row, False)
            want = [e for e in order.tolist() if e not in known or e == true]
            assert kept[i][:len(want)].tolist() == want


def test_predict_refusals():
    c, cfg, m, ev, B, S, row_of = _setup()
    with pytest.raises(ValueError, match="KGE_TOPK_MAX"):
        ev.predict_tails([0], [0], topk=1025)
    with pytest.raises(ValueError, match="KGE_TOPK_MAX"):
        ev.predict_rels([0], [0], topk=0)
    from pykg2vec_amd.kgmeta import ProjectionModel
    from pykg2vec_amd.projection import TuckER
    tucker = TuckER(tot_entity=c.E, tot_relation=c.R, ent_hidden_size=8, rel_hidden_size=4, lmbda=0.0, input_dropout=0.3, hidden_dropout1=0.4,
                    hidden_dropout2=0.5)
    assert isinstance(tucker, ProjectionModel) and tucker.higher_is_better and not m.higher_is_better
    ev.model = tucker
    with pytest.raises(ValueError, match="projection"):
        ev.predict_rels([0], [1], topk=3)


def test_predict_rels_scores_every_relation_through_forward():
    c, cfg, m, ev, B, S, row_of = _setup()
    G = torch.from_numpy(np.round(np.random.default_rng(9).normal(size=(c.E, c.R, 3)) * 2).astype(np.float32))
    m.forward = lambda h, r, t: G[h, r, t % 3]
    h, t = np.asarray([3, 1, 4, 1, 5]), np.asarray([9, 2, 6, 5, 3])
    ev.PREDICT_SCRATCH_BYTES = 2 * c.R * ev.PREDICT_ROW_ITEM_BYTES
    ids, vals = ev.predict_rels(h, t, topk=min(c.R, 6))
    assert B.chunks == [2, 2, 1]
    rows = np.stack([G[h[i], :, t[i] % 3].numpy() for i in range(len(h))])
    want = topk_ref.topk_ref(rows, min(c.R, 6))
    assert np.array_equal(ids.numpy(), want[0]) and np.array_equal(vals.numpy(), want[1])


def test_trainer_infer_returns_names_in_prediction_order_and_drops_padding():
    from pykg2vec_amd.trainer import Trainer
    c, cfg, m, ev, B, S, row_of = _setup()
    tr = Trainer(m, cfg, backend=B)
    tr.build_model()
    h, r, t = (int(x) for x in c.test[0])
    hr_t, tr_h = c.filters()
    row = S[row_of(np.asarray([[h, r, 0]]), 0)][0]
    got = tr.infer_tails(h, r, topk=5)
    want = topk_ref.row_order(row, False)[:5].tolist()
    assert list(got) == want and got == {e: "e%d" % e for e in want}
    got = tr.infer_tails(h, r, topk=c.E, filtered=True)       # more places than live candidates: the -1 padding is dropped
    assert list(got) == [e for e in topk_ref.row_order(row, False).tolist() if e not in hr_t[(h, r)]]
    row = S[row_of(np.asarray([[0, r, t]]), 1)][0]
    assert list(tr.infer_heads(r, t, topk=4)) == topk_ref.row_order(row, False)[:4].tolist()
    G = torch.from_numpy(np.random.default_rng(2).normal(size=(c.R,)).astype(np.float32))
    m.forward = lambda hh, rr, tt: G[rr]
    got = tr.infer_rels(h, t, topk=3)
    want = np.argsort(G.numpy(), kind="stable")[:3].tolist()
    assert list(got) == want and got == {i: "r%d" % i for i in want}
