"""Relation ranking on the GPU: kge_rank_relations (csrc/kge_relations.hip) against the composed path it replaces -- the R - 1 other
relations of every query expanded to explicit triples, scored by kernels.score_forward and counted in numpy (tests/relations_ref.py)
-- and kge_relation_csr_* (csrc/kge_index.hip) against the numpy builder.  The fused kernel's scores are defined as
kge_score_forward's bit for bit, so counts are compared with array_equal: nothing here has a tolerance except the comparison with
float64, which uses golden_util.rank_band_ok's band around the true score."""
import numpy as np
import pytest
import torch

import hip_util
import kge_oracle as ko
import relations_ref as rr
from golden_util import Case, rank_band_ok

pytestmark = pytest.mark.gpu

ROW_CASES = ["transe_l1", "transe_l2", "transh_l1", "transd_l1", "transm_l1", "rotate", "distmult", "complex", "analogy", "cp", "simple",
             "simple_ignr", "quate", "kg2e"]     # the thirteen row-kernel models (TransE in both norms)
E0, N0 = 211, 12                                  # the smallest shapes: entities and queries unless a test says otherwise


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    """Other test modules of this suite leave KGE_* A/B switches set in the process environment: every test here starts without them."""
    from test_tucker_model import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def K():
    from pykg2vec_amd import kernels
    return kernels


def fused(desc, q, s_off=None, s_ids=None, **kw):
    d = hip_util.dev
    return K().rank_relations(desc, d(q), None if s_off is None else d(s_off), None if s_ids is None else d(s_ids, torch.int32), **kw).cpu().numpy()


def score_fn(desc):
    d = hip_util.dev
    return lambda h, r, t: K().score_forward(desc, d(h), d(r), d(t)).cpu().numpy()


def composed(desc, q, R, s_off=None, s_ids=None):
    return rr.rank_relations_ref(score_fn(desc), q, R, s_off, s_ids)


def queries(rng, n, E, R):
    return np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1).astype(np.int64)


def known_for(rng, q, R):
    """Known triples in which every query's pair carries its own relation, about a third of the others, and a duplicate."""
    rows = [q]
    for h, r, t in q.tolist():
        other = rng.permutation(R)[:max(1, R // 3)]
        rows.append(np.stack([np.full(len(other), h), other, np.full(len(other), t)], 1))
    known = np.concatenate(rows).astype(np.int64)
    return np.concatenate([known, known[:3]])[rng.permutation(len(known) + 3)]


def check_exact(desc, q, R, rng):
    lists = rr.known_relations(known_for(rng, q, R), q)
    assert all(int(r) in x for x, r in zip(lists, q[:, 1]))
    if R > 3:
        assert sum(len(x) > 1 for x in lists) >= 3                   # several pairs carry more than one relation
    s_off, s_ids = rr.csr_of(lists)
    got = fused(desc, q, s_off, s_ids, skip_sorted=True)
    want = composed(desc, q, R, s_off, s_ids)
    assert got.dtype == np.int32 and got.shape == (4, len(q))
    assert np.array_equal(got, want), (np.argwhere(got != want)[:8], got[:, :8], want[:, :8])
    plain = fused(desc, q)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[2], got[2])
    assert np.array_equal(plain[1], plain[0]) and np.array_equal(plain[3], plain[2])
    assert (got[1] <= got[0]).all() and (got[3] <= got[2]).all() and (got[0] + got[2] <= R - 1).all()
    if R > 3:
        assert (got[1] + got[3] < got[0] + got[2]).any()            # the filter left live relations out
    return got


_MODELS = {}


def golden_model(name):
    if name not in _MODELS:
        c = Case(name)
        _MODELS[name] = (c, hip_util.model_from_case(c))
    return _MODELS[name]


def params_model(model, l1, d, E, R, rng):
    kw = dict(margin=6.0) if model == "rotate" else {}
    P = ko.init_params(model, rng, tot_entity=E, tot_relation=R, hidden_size=d, **kw)
    hp = dict(hidden_size=d, margin=6.0 if model == "rotate" else 1.0, lmbda=0.01, alpha=1.0)
    if l1 is not None:
        hp["l1_flag"] = l1
    return hip_util.model_from_params(model, P, hp, E, R), P, hp


@pytest.mark.parametrize("name", ROW_CASES)
def test_fused_path_is_the_composed_path_exactly(name):
    """1: every row-kernel model on its golden tables, with and without skip segments, pairs that carry several relations."""
    c, m = golden_model(name)
    q = np.ascontiguousarray(c.test[:N0], dtype=np.int64)
    check_exact(m.make_desc(), q, c.R, np.random.default_rng(1))


@pytest.mark.parametrize("model,l1", [("transe", True), ("transe", False), ("complex", None)])
def test_relation_counts_around_the_chunk_size(model, l1):
    """2: R = 1 (nothing to rank against), 2, and around the multiples of KGE_REL_CHUNK."""
    CH = K().REL_CHUNK
    for R in (1, 2, CH - 1, CH, CH + 1, 2 * CH + 3):
        rng = np.random.default_rng(R)
        m, _, _ = params_model(model, l1, 20, E0, R, rng)
        q = queries(rng, N0, E0, R)
        q[0, 1], q[1, 1] = 0, R - 1                                  # the true relation at both ends of the range
        got = check_exact(m.make_desc(), q, R, rng)
        if R == 1:
            assert not got.any()


GEOMETRY_CASES = ([("transe", l1, d) for l1 in (True, False) for d in (20, 50, 100, 200, 300, 1000)] +
                  [("complex", None, d) for d in (20, 50, 100, 200, 300, 1000)] + [("transe", True, 2048), ("rotate", None, 1000)])


@pytest.mark.parametrize("model,l1,d", GEOMETRY_CASES)
def test_every_geometry(model, l1, d):
    """3: all seven (G, NCH) pairs, including row lengths that do not fill the last chunk of registers; R = CH + 1."""
    rng = np.random.default_rng(d)
    R = K().REL_CHUNK + 1
    m, _, _ = params_model(model, l1, d, E0, R, rng)
    check_exact(m.make_desc(), queries(rng, N0, E0, R), R, rng)


@pytest.mark.parametrize("n_known", [1, 2047, 2048, 2049])
def test_device_csr_is_the_numpy_builder(n_known):
    """4: kge_relation_csr_* at the sort's tile edge, with a long run, an absent pair, a duplicate triple and the top ids."""
    from pykg2vec_amd.evaluator import build_relation_csr_from_triples
    rng = np.random.default_rng(n_known)
    E, R = 1 << 24, 1 << 16
    if n_known == 1:
        known = np.asarray([[3, R - 1, 4]], dtype=np.int64)
    else:
        known = np.stack([rng.integers(12, size=n_known), rng.integers(R, size=n_known), rng.integers(12, size=n_known)], 1).astype(np.int64)
        run = np.concatenate([[0, R - 1], 1 + rng.permutation(R - 2)[:78]])      # 80 relations for the pair (3, 4), r = 65535 among them
        known[:80] = np.stack([np.full(80, 3), run, np.full(80, 4)], 1)
        known[100] = known[101]                                                   # a triple present in two splits
        known[102] = known[5]
        known[200] = [E - 1, R - 1, E - 1]                                        # the key of all ones
        known[201] = [E - 1, 7, E - 1]
        known = known[rng.permutation(n_known)]
    pairs = [[3, 0, 4], [4, 0, 3], [200, 1, 201], [E - 1, 2, E - 1], [0, 0, 0], [11, 5, 11]] + known[:6].tolist()
    q = np.asarray(pairs, dtype=np.int64)
    want_off, want_ids = build_relation_csr_from_triples(q, known, E)
    lists = rr.known_relations(known, q)
    assert [want_ids[want_off[i]:want_off[i + 1]].tolist() for i in range(len(q))] == lists
    assert lists[2] == [] and lists[0][-1] == R - 1 and (n_known == 1 or (len(lists[0]) > 64 and lists[3] == [7, R - 1]))
    off, ids = K().relation_csr_build(hip_util.dev(known), hip_util.dev(q), E, R)
    assert off.dtype == torch.int64 and ids.dtype == torch.int32
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(ids.cpu().numpy(), want_ids)


def test_ties_are_counted_bit_for_bit_and_a_nan_row_counts_nowhere():
    """5: two identical relation rows, DistMult on tables of multiples of 1/4, a NaN relation row."""
    rng = np.random.default_rng(5)
    R, d = 9, 20
    m, P, hp = params_model("transe", True, d, E0, R, rng)
    P = {k: v.copy() for k, v in P.items()}
    P["rel_embeddings"][2] = P["rel_embeddings"][1]              # relations 1 and 2 are the same row
    P["rel_embeddings"][5] = np.nan
    m = hip_util.model_from_params("transe", P, hp, E0, R)
    desc = m.make_desc()
    q = queries(rng, N0, E0, R)
    q[:4, 1] = [1, 2, 5, 1]
    skip = rr.csr_of([[1, 2]] * N0)                              # the twin relation is known for every pair
    got = fused(desc, q, *skip, skip_sorted=True)
    assert np.array_equal(got, composed(desc, q, R, *skip))
    assert (got[2, [0, 1, 3]] == 1).all() and (got[3, [0, 1, 3]] == 0).all()      # exactly the twin ties, and the filter leaves it out
    assert not got[:, 2].any()                                   # a NaN true score: nothing is below it, nothing equals it
    s = score_fn(desc)
    for i in (0, 1, 3, 4, 7):                                    # the optimistic end: strictly better relations only; the NaN row is none
        row = s(np.full(R, q[i, 0]), np.arange(R), np.full(R, q[i, 2]))
        assert np.isnan(row[5]) and got[0, i] == int((row < row[q[i, 1]]).sum()) and got[0, i] + got[2, i] <= R - 2
    P2 = {k: (rng.integers(-2, 3, size=v.shape) / 4).astype(np.float32)
          for k, v in ko.init_params("distmult", rng, tot_entity=97, tot_relation=40, hidden_size=d).items()}
    dm = hip_util.model_from_params("distmult", P2, dict(hidden_size=d, lmbda=0.01), 97, 40)
    q2 = queries(rng, 16, 97, 40)
    got2 = check_exact(dm.make_desc(), q2, 40, rng)
    assert got2[2].max() > 0 and got2[3].max() > 0               # tie groups exist, raw and filtered


def test_result_does_not_depend_on_the_execution_order():
    """6: more items than the launch has groups (the grid-stride loop runs more than once); two calls give identical tensors."""
    rng = np.random.default_rng(8)
    E, R, d, n = 64, 3, 20, 20000
    m, _, _ = params_model("transe", True, d, E, R, rng)
    desc = m.make_desc()
    q = queries(rng, n, E, R)
    d_ = hip_util.dev
    a = K().rank_relations(desc, d_(q))
    b = K().rank_relations(desc, d_(q))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), composed(desc, q, R))


@pytest.mark.parametrize("name", ["rescal", "ntn", "transr_l1", "slm", "hole", "octonione", "convkb", "murp"])
def test_via_forward_path(name):
    """7: the models without row kernels rank through their own forward + kge_rank_lists_from_scores, in one chunk and in several."""
    from test_hip_candidates import VIA_FORWARD
    from test_hip_link_prediction import load
    from pykg2vec_amd.evaluator import Evaluator
    assert name in VIA_FORWARD
    m, E, R, train, valid, test, hp, kw = load(name)
    m.eval()
    cfg = hip_util.make_config(E, R, hp, train, valid, test, **kw)
    ev = Evaluator(m, cfg)
    n = min(N0, len(test))
    q = np.ascontiguousarray(test[:n], dtype=np.int64)
    d = hip_util.dev
    fwd = lambda h, r, t: m.forward(d(h), d(r), d(t)).detach().cpu().numpy()
    known = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1, 3) for x in (train, valid, test)])
    with torch.no_grad():
        for _ in range(8):      # RESCAL's forward renormalises its tables in place: iterate to the fixed point
            before = [p.detach().clone() for p in m.parameters()]
            fwd(q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
            if all(torch.equal(a, b) for a, b in zip(before, m.parameters())):
                break
        want = rr.rank_relations_ref(fwd, q, R, *rr.csr_of(rr.known_relations(known, q)), largest=bool(m.higher_is_better))
        got, ties = ev.rank_relations(q, n, return_ties=True)
    assert fwd(q[:1, 0].copy(), q[:1, 1].copy(), q[:1, 2].copy()).dtype == (np.float64 if name == "murp" else np.float32)
    assert np.array_equal(got.cpu().numpy(), want[:2]) and np.array_equal(ties.cpu().numpy(), want[2])
    budget = ev.PREDICT_SCRATCH_BYTES
    try:
        ev.PREDICT_SCRATCH_BYTES = 5 * max(1, R - 1) * ev.CANDIDATE_ENTRY_BYTES     # five queries per chunk: three chunks
        assert torch.equal(ev.rank_relations(q, n), got)
    finally:
        ev.PREDICT_SCRATCH_BYTES = budget


@pytest.mark.parametrize("name", ["transe_l1", "transe_l2", "rotate", "complex", "quate"])
def test_against_float64(name):
    """8: ranks from the float64 oracle may differ only by relations inside the fp32 band around the true score."""
    c, m = golden_model(name)
    n = 24
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    params = c.params()
    got = fused(m.make_desc(), q)
    differ = 0
    for i in range(n):
        row = ko.score(c.model, params, np.full(c.R, q[i, 0]), np.arange(c.R), np.full(c.R, q[i, 2]), dtype=np.float64, **c.hp)
        ref = int((row < row[q[i, 1]]).sum())
        ok, near = rank_band_ok(row, int(q[i, 1]), got[0, i], ref)
        assert ok, (name, i, got[0, i], ref, near)
        differ += int(got[0, i] != ref)
    hip_util.record_max("relations_parity", "%s.rank_differs_from_float64_fraction" % name, differ / n)


def test_metrics_device_filter_and_debug_mode():
    """9: test_relations returns the metrics of the composed counts (filter built on the device); the debug id mode refuses an
    unsorted skip segment and ids out of range; off, nothing is checked."""
    from pykg2vec_amd import _lib
    from pykg2vec_amd.evaluator import Evaluator
    c, m = golden_model("distmult")
    extra = c.test[:N0].copy()
    extra[:, 1] = (extra[:, 1] + 1 + np.arange(N0) % 3) % c.R        # other relations known for the test pairs
    train = np.concatenate([c.train, extra])
    cfg = hip_util.make_config(c.E, c.R, c.hp, train, c.valid, c.test)
    ev = Evaluator(m, cfg)
    desc = m.make_desc()
    n = 24
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    known = np.concatenate([train, c.valid, c.test])
    want = composed(desc, q, c.R, *rr.csr_of(rr.known_relations(known, q)))
    assert (want[1] < want[0]).any()
    got = ev.test_relations(q, n, epoch=0)
    assert rr.same_metrics(got, rr.metrics(want[:2], cfg.hits)), (got, rr.metrics(want[:2], cfg.hits))
    assert np.array_equal(ev.relation_tie_counts, want[2])
    ranks = ev.rank_relations(q, n)
    assert ranks.is_cuda and np.array_equal(ranks.cpu().numpy(), want[:2])
    d = hip_util.dev
    good = (d(np.asarray([0, 2, 2, 4, 5])), d(np.asarray([3, 6, 2, 2, 4]), torch.int32))        # ascending, equal ids allowed
    bad = (d(np.asarray([0, 2, 2, 4, 5])), d(np.asarray([3, 6, 5, 2, 4]), torch.int32))         # segment 2 descends at position 3
    call = lambda qq=q[:4], skip=good: K().rank_relations(desc, d(qq), skip[0], skip[1], skip_sorted=True)
    was = K().debug_enabled()
    K().set_debug(True)
    try:
        ok = call().cpu().numpy()
        with pytest.raises(_lib.KgeHipError, match="ascending.*position 3"):
            call(skip=bad)
        far = q[:4].copy()
        far[2, 0] = c.E
        with pytest.raises(_lib.KgeHipError, match="head id out of range"):
            call(qq=far)
        far = q[:4].copy()
        far[1, 1] = c.R
        with pytest.raises(_lib.KgeHipError, match="relation id out of range.* %d not in" % c.R):
            call(qq=far)
    finally:
        K().set_debug(was)
    assert np.array_equal(call().cpu().numpy(), ok)
    tucker = __import__("test_hip_link_prediction").load("tucker")
    with pytest.raises(ValueError, match="projection"):
        Evaluator(tucker[0], hip_util.make_config(tucker[1], tucker[2], tucker[6], tucker[3], tucker[4], tucker[5], **tucker[7])).rank_relations(tucker[5][:4], 4)
