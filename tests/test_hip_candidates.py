"""Candidate-list ranking on the GPU: kge_rank_candidates (csrc/kge_candidates.hip) against the composed path it replaces -- the live
list entries expanded to explicit triples, scored by kernels.score_forward and counted in numpy (tests/candidates_ref.py).  The fused
kernel's scores are defined as kge_score_forward's bit for bit, so counts are compared with array_equal: nothing here has a tolerance
except the comparisons with float64 and with the dense sweep, which use golden_util.rank_band_ok's band around the true score."""
import numpy as np
import pytest
import torch

import candidates_ref as cr
import hip_util
import kge_oracle as ko
from golden_util import Case, rank_band_ok

pytestmark = pytest.mark.gpu

ROW_CASES = ["transe_l1", "transe_l2", "transh_l1", "transd_l1", "transm_l1", "rotate", "distmult", "complex", "analogy", "cp", "simple",
             "simple_ignr", "quate", "kg2e"]     # the thirteen row-kernel models (TransE in both norms)


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    """Other test modules of this suite leave KGE_* A/B switches set in the process environment: every test here starts without them."""
    from test_tucker_model import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def K():
    from pykg2vec_amd import kernels
    return kernels


def lengths():
    CH = K().CAND_CHUNK
    return [0, 1, CH - 1, CH, CH + 1, 2 * CH + 3]


def make_lists(rng, q, side, E, lens):
    """One list per query with the given lengths: random ids with the true id, a duplicate, -1 and ids >= E among them."""
    true = q[:, 0 if side else 2]
    lists = []
    for i, L in enumerate(lens):
        x = rng.integers(E, size=L)
        if L > 3:
            x[0], x[1], x[2], x[3] = true[i], x[L - 1], -1, E + i
        if L > 70:
            x[66], x[67], x[68] = true[i], -1, E
        if L == 1 and i % 2:
            x[0] = true[i]
        lists.append(x.tolist())
    return lists


def skip_lists(rng, lists, E, unsorted=True):
    """Per query about a third of its list + strangers, in random order with a duplicate."""
    out = []
    for x in lists:
        live = [e for e in x if 0 <= e < E]
        pick = list(rng.permutation(live)[:len(live) // 3]) + rng.integers(E, size=3).tolist()
        if pick:
            pick.append(pick[0])
        out.append([int(e) for e in (rng.permutation(pick) if unsorted else sorted(pick))])
    return out


def fused(desc, q, side, off, ids, loq=None, s_off=None, s_ids=None, **kw):
    d = hip_util.dev
    return K().rank_candidates(desc, d(q), side, d(off), d(ids, torch.int32), None if loq is None else d(loq), None if s_off is None else d(s_off),
                               None if s_ids is None else d(s_ids, torch.int32), **kw).cpu().numpy()


def score_fn(desc):
    d = hip_util.dev
    return lambda h, r, t: K().score_forward(desc, d(h), d(r), d(t)).cpu().numpy()


def composed(desc, q, side, off, ids, E, loq=None, s_off=None, s_ids=None):
    return cr.rank_candidates_ref(score_fn(desc), q, side, off, ids, E, loq, s_off, s_ids)


def check_exact(desc, q, E, rng, lens):
    for side in (0, 1):
        lists = make_lists(rng, q, side, E, lens)
        off, ids = cr.csr_of(lists)
        s_off, s_ids = cr.csr_of(skip_lists(rng, lists, E))
        got = fused(desc, q, side, off, ids, None, s_off, s_ids)
        want = composed(desc, q, side, off, ids, E, None, s_off, s_ids)
        assert got.dtype == np.int32 and np.array_equal(got, want), (side, np.argwhere(got != want)[:8], got[:, :8], want[:, :8])
        plain = fused(desc, q, side, off, ids)
        assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], plain[0]) and np.array_equal(plain[3], plain[2])
        assert (got[1] <= got[0]).all() and (got[1] + got[3] < got[0] + got[2]).any()     # the filter left live entries out


_MODELS = {}


def golden_model(name):
    if name not in _MODELS:
        c = Case(name)
        m = hip_util.model_from_case(c)
        _MODELS[name] = (c, m)
    return _MODELS[name]


@pytest.mark.parametrize("name", ROW_CASES)
def test_fused_path_is_the_composed_path_exactly(name):
    """1: every row-kernel model, both sides, list lengths around the chunk size, dead entries of every kind, with and without skip lists."""
    c, m = golden_model(name)
    lens = lengths() * 2
    q = np.ascontiguousarray(c.test[:len(lens)], dtype=np.int64)
    assert len(q) == len(lens)
    check_exact(m.make_desc(), q, c.E, np.random.default_rng(1), lens)


GEOMETRY_CASES = ([("transe", l1, d) for l1 in (True, False) for d in (20, 50, 100, 200, 300, 1000)] +
                  [("complex", None, d) for d in (20, 50, 100, 200, 300, 1000)] + [("transe", True, 2048), ("rotate", None, 1000)])


@pytest.mark.parametrize("model,l1,d", GEOMETRY_CASES)
def test_every_geometry(model, l1, d):
    """2: all seven (G, NCH) pairs, including row lengths that do not fill the last chunk of registers."""
    rng = np.random.default_rng(d)
    E, R = 211, 5
    kw = dict(margin=6.0) if model == "rotate" else {}
    P = ko.init_params(model, rng, tot_entity=E, tot_relation=R, hidden_size=d, **kw)
    hp = dict(hidden_size=d, margin=6.0 if model == "rotate" else 1.0, lmbda=0.01, alpha=1.0)
    if l1 is not None:
        hp["l1_flag"] = l1
    m = hip_util.model_from_params(model, P, hp, E, R)
    lens = lengths()
    q = np.stack([rng.integers(E, size=len(lens)), rng.integers(R, size=len(lens)), rng.integers(E, size=len(lens))], 1).astype(np.int64)
    check_exact(m.make_desc(), q, E, rng, lens)


@pytest.mark.parametrize("name", ["transe_l1", "transe_l2", "rotate", "complex", "quate"])
def test_against_float64(name):
    """3: ranks from the float64 oracle over the same lists may differ only by candidates inside the fp32 band around the true score."""
    c, m = golden_model(name)
    rng = np.random.default_rng(3)
    n = 24
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    params = c.params()
    f64 = lambda h, r, t: ko.score(c.model, params, h, r, t, dtype=np.float64, **c.hp)
    differ = total = 0
    for side in (0, 1):
        lists = [rng.integers(c.E, size=130).tolist() for _ in range(n)]
        off, ids = cr.csr_of(lists)
        got = fused(m.make_desc(), q, side, off, ids)
        entries = cr.live_entries(q, side, off, ids, None, c.E)
        h, r, t, seg = cr.expand(q, side, entries)
        s, s_true = f64(h, r, t), f64(q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
        for i in range(n):
            row = np.concatenate([s[seg[i]:seg[i + 1]], [s_true[i]]])
            ref = int((row[:-1] < row[-1]).sum())
            ok, near = rank_band_ok(row, len(row) - 1, got[0, i], ref)
            assert ok, (name, side, i, got[0, i], ref, near)
            differ += int(got[0, i] != ref)
            total += 1
    hip_util.record_max("candidates_parity", "%s.rank_differs_from_float64_fraction" % name, differ / total)


def test_filter_edge_cases():
    """4: empty segment, a segment holding every candidate, a segment holding the true id, the wrapper's sort, skip_sorted."""
    c, m = golden_model("transe_l1")
    desc = m.make_desc()
    rng = np.random.default_rng(4)
    n = 8
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    lists = [rng.integers(c.E, size=70).tolist() for _ in range(n)]
    off, ids = cr.csr_of(lists)
    skips = [[] for _ in range(n)]
    skips[1] = list(lists[1])                              # every candidate: filtered counts 0
    skips[2] = [int(q[2, 2])]                              # the true id alone: ignored
    plain = fused(desc, q, 0, off, ids)
    j = max((3, 5, 6, 7), key=lambda i: plain[0, i])         # a query whose true entity has better candidates in its list
    assert plain[0, j] > 0
    skips[j] = list(rng.permutation(lists[j] * 2))         # every candidate again, unsorted and duplicated: the wrapper sorts
    skips[4] = [c.E + 3, -1] + lists[4][:5]                # out-of-range ids in the skip list
    s_off, s_ids = cr.csr_of([[int(e) for e in s] for s in skips])
    want = composed(desc, q, 0, off, ids, c.E, None, s_off, s_ids)
    got = fused(desc, q, 0, off, ids, None, s_off, s_ids)
    assert np.array_equal(got, want)
    assert got[1, 1] == 0 and got[3, 1] == 0 and got[0, 1] > 0
    assert np.array_equal(got[1, [0, 2]], got[0, [0, 2]]) and np.array_equal(got[0], plain[0])
    assert got[1, j] == 0 and got[3, j] == 0 and got[0, j] > 0
    sorted_off, sorted_ids = cr.csr_of([sorted(int(e) for e in s) for s in skips])
    assert np.array_equal(fused(desc, q, 0, off, ids, None, sorted_off, sorted_ids, skip_sorted=True), want)
    # the wrapper's sort keeps the CSR layout
    sk = K().sort_skip_segments(hip_util.dev(s_off), hip_util.dev(s_ids, torch.int32)).cpu().numpy()
    assert np.array_equal(sk, sorted_ids)


def test_shared_lists():
    """5: list_of_query maps many queries to few lists (the type-constrained shape) = the same lists replicated per query."""
    c, m = golden_model("complex")
    desc = m.make_desc()
    rng = np.random.default_rng(5)
    n = 40
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    few = [rng.integers(c.E, size=L).tolist() for L in (0, 5, 64, 150)]
    loq = rng.integers(len(few), size=n)
    off, ids = cr.csr_of(few)
    roff, rids = cr.csr_of([few[k] for k in loq])
    for side in (0, 1):
        got = fused(desc, q, side, off, ids, loq)
        assert np.array_equal(got, fused(desc, q, side, roff, rids))
        assert np.array_equal(got, composed(desc, q, side, roff, rids, c.E))


def test_full_list_is_the_full_sweep():
    """6: every list = arange(E): the counts are eval_ranks_via_forward's ranks exactly, and rank_all's inside the fp32 band."""
    from pykg2vec_amd.evaluator import CandidateLists, Evaluator, build_filter_csr
    c, m = golden_model("transe_l1")
    desc = m.make_desc()
    n = 32
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    hr_t, tr_h = c.filters()
    t_off, t_ids, h_off, h_ids = build_filter_csr(q, hr_t, tr_h)
    off, ids = np.asarray([0, c.E], dtype=np.int64), np.arange(c.E, dtype=np.int32)
    loq = np.zeros(n, dtype=np.int64)
    ct = fused(desc, q, 0, off, ids, loq, t_off, t_ids)
    ch = fused(desc, q, 1, off, ids, loq, h_off, h_ids)
    d = hip_util.dev
    via = K().eval_ranks_via_forward(desc, d(q), d(t_off), d(t_ids, torch.int32), d(h_off), d(h_ids, torch.int32)).cpu().numpy()
    assert np.array_equal(np.stack([ch[0], ct[0], ch[1], ct[1]]), via)
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    ev = Evaluator(m, cfg)
    full = CandidateLists(off, ids, loq)
    got = ev.rank_candidates(q, n, full, full).cpu().numpy()
    assert np.array_equal(got, via)
    dense = ev.rank_all(q, n).cpu().numpy()
    rows = K().eval_sweep_scores(desc, d(q)).cpu().numpy()
    for i in range(n):
        for row, true, pair in ((rows[2 * i], q[i, 2], (1, 3)), (rows[2 * i + 1], q[i, 0], (0, 2))):
            for k in pair:
                assert rank_band_ok(row, int(true), got[k, i], dense[k, i])[0], (i, k, got[k, i], dense[k, i])


def test_ties_are_counted_bit_for_bit_and_ranks_are_the_optimistic_end():
    """7: the saturated SimplE case and DistMult on tables of multiples of 1/4."""
    c, m = golden_model("simple_ties")
    rng = np.random.default_rng(7)
    n = 16
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    lists = [rng.integers(c.E, size=100).tolist() for _ in range(n)]
    off, ids = cr.csr_of(lists)
    E, R, d = 97, 4, 20
    P = {k: (rng.integers(-2, 3, size=v.shape) / 4).astype(np.float32)
         for k, v in ko.init_params("distmult", rng, tot_entity=E, tot_relation=R, hidden_size=d).items()}
    dm = hip_util.model_from_params("distmult", P, dict(hidden_size=d, lmbda=0.01), E, R)
    q2 = np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1).astype(np.int64)
    off2, ids2 = cr.csr_of([rng.integers(E, size=100).tolist() for _ in range(n)])
    for desc, qq, o, i, EE in ((m.make_desc(), q, off, ids, c.E), (dm.make_desc(), q2, off2, ids2, E)):
        for side in (0, 1):
            got = fused(desc, qq, side, o, i)
            assert np.array_equal(got, composed(desc, qq, side, o, i, EE))
            assert got[2].max() > 0     # tie groups exist, and rows 0 / 1 count the strictly better candidates only


def test_result_does_not_depend_on_the_execution_order():
    """8: more items than the launch has groups (the grid-stride loop runs more than once); two calls give identical tensors."""
    rng = np.random.default_rng(8)
    E, R, d, n = 64, 3, 20, 20000
    P = ko.init_params("transe", rng, tot_entity=E, tot_relation=R, hidden_size=d)
    m = hip_util.model_from_params("transe", P, dict(hidden_size=d, l1_flag=True, margin=1.0), E, R)
    desc = m.make_desc()
    q = np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1).astype(np.int64)
    table = rng.integers(E, size=(n, 1))
    off, ids = cr.to_csr(table)
    a, b = fused(desc, q, 0, off, ids), fused(desc, q, 0, off, ids)
    assert np.array_equal(a, b)
    s_true = score_fn(desc)(q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
    s = score_fn(desc)(q[:, 0].copy(), q[:, 1].copy(), table[:, 0].copy())
    live = table[:, 0] != q[:, 2]
    assert np.array_equal(a[0], ((s < s_true) & live).astype(np.int32)) and np.array_equal(a[2], ((s == s_true) & live).astype(np.int32))


VIA_FORWARD = ["rescal", "ntn", "transr_l1", "slm", "hole", "octonione", "convkb", "murp"]


@pytest.mark.parametrize("name", VIA_FORWARD)
def test_via_forward_path(name):
    """9: the models without row kernels rank through their own forward + kge_rank_lists_from_scores."""
    from test_hip_link_prediction import load
    from pykg2vec_amd.evaluator import Evaluator
    m, E, R, train, valid, test, hp, kw = load(name)
    m.eval()
    cfg = hip_util.make_config(E, R, hp, train, valid, test, **kw)
    ev = Evaluator(m, cfg)
    n = min(12, len(test))
    q = np.ascontiguousarray(test[:n], dtype=np.int64)
    rng = np.random.default_rng(9)
    d = hip_util.dev
    fwd = lambda h, r, t: m.forward(d(h), d(r), d(t)).detach().cpu().numpy()
    with torch.no_grad():
        for _ in range(8):      # RESCAL's forward renormalises its tables in place: iterate to the fixed point
            before = [p.detach().clone() for p in m.parameters()]
            fwd(q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())
            if all(torch.equal(a, b) for a, b in zip(before, m.parameters())):
                break
        tables = []
        for side in (0, 1):
            t = rng.integers(E, size=(n, 11))
            t[:, 0], t[:, 1], t[::2, 2], t[1::2, 3] = q[:, 0 if side else 2], t[:, 4], -1, E + 1
            tables.append(t)
        hr_t, tr_h = cfg.knowledge_graph.cache["hr_t"], cfg.knowledge_graph.cache["tr_h"]
        want = []
        for side in (0, 1):
            known = [sorted(tr_h[(int(t), int(r))]) if side else sorted(hr_t[(int(h), int(r))]) for h, r, t in q]
            off, ids = cr.to_csr(tables[side])
            want.append(cr.rank_candidates_ref(fwd, q, side, off, ids, E, None, *cr.csr_of(known), largest=bool(m.higher_is_better)))
        ct, ch = want
        got, ties = ev.rank_candidates(q, n, tables[0], tables[1], return_ties=True)
    assert fwd(q[:1, 0].copy(), q[:1, 1].copy(), q[:1, 2].copy()).dtype == (np.float64 if name == "murp" else np.float32)
    assert np.array_equal(got.cpu().numpy(), np.stack([ch[0], ct[0], ch[1], ct[1]]))
    assert np.array_equal(ties.cpu().numpy(), np.stack([ch[2], ct[2]]))
    budget = ev.PREDICT_SCRATCH_BYTES
    try:
        ev.PREDICT_SCRATCH_BYTES = 3 * 11 * ev.CANDIDATE_ENTRY_BYTES     # four chunks
        assert torch.equal(ev.rank_candidates(q, n, tables[0], tables[1]), got)
    finally:
        ev.PREDICT_SCRATCH_BYTES = budget


def test_projection_models_raise_and_count_kernel_handles_both_dtypes():
    """9: projection models are refused; kge_rank_lists_from_scores on float32 and float64 segments with an empty segment and NaNs."""
    from test_hip_link_prediction import load
    from pykg2vec_amd.evaluator import Evaluator
    from pykg2vec_amd import _lib
    m, E, R, train, valid, test, hp, kw = load("tucker")
    ev = Evaluator(m, hip_util.make_config(E, R, hp, train, valid, test, **kw))
    with pytest.raises(ValueError, match="projection"):
        ev.rank_candidates(test[:4], 4, np.zeros((4, 3), np.int64), np.zeros((4, 3), np.int64))
    c, tm = golden_model("transe_l1")
    with pytest.raises(_lib.KgeHipError, match="via-forward"):
        K().rank_candidates(ev.K.model_desc(m), hip_util.dev(test[:4]), 0, hip_util.dev([0, 0, 0, 0, 0]), hip_util.dev([0], torch.int32))
    rng = np.random.default_rng(10)
    seg = np.asarray([0, 0, 1, 66, 200, 200, 333], dtype=np.int64)
    for dtype in (np.float32, np.float64):
        s = (np.round(rng.normal(size=333) * 2) / 2).astype(dtype)
        s[rng.random(333) < 0.1] = np.nan
        truth = np.asarray([0.5, 0.0, -0.5, np.nan, 1.0, 0.0], dtype=dtype)
        flags = rng.integers(0, 4, size=333).astype(np.uint8)
        for largest in (False, True):
            for f in (flags, None):
                got = K().rank_lists_from_scores(torch.from_numpy(s).cuda(), torch.from_numpy(truth).cuda(), hip_util.dev(seg),
                                                 None if f is None else torch.from_numpy(f).cuda(), largest=largest).cpu().numpy()
                assert np.array_equal(got, cr.rank_lists_from_scores_ref(s, truth, seg, f, largest)), (dtype, largest)
                assert (got[:, [0, 3, 4]] == 0).all() and got[0].max() > 0


def test_metrics_of_the_three_protocols():
    """10: test_candidates / test_type_constrained / test_sampled return the MetricCalculator dict of the composed path's counts."""
    from pykg2vec_amd.evaluator import Evaluator, build_filter_csr, build_type_constraints
    c, m = golden_model("distmult")
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, c.valid, c.test)
    ev = Evaluator(m, cfg)
    desc = m.make_desc()
    n = 24
    q = np.ascontiguousarray(c.test[:n], dtype=np.int64)
    rng = np.random.default_rng(11)
    tables = [rng.integers(-1, c.E + 2, size=(n, 70)) for _ in (0, 1)]
    t_off, t_ids, h_off, h_ids = build_filter_csr(q, *c.filters())
    per = [composed(desc, q, side, *cr.to_csr(tables[side]), c.E, None, *((h_off, h_ids) if side else (t_off, t_ids))) for side in (0, 1)]
    want = cr.metrics(np.stack([per[1][0], per[0][0], per[1][1], per[0][1]]))
    got = ev.test_candidates(q, n, tables[0], tables[1], epoch=0)
    assert set(got) == {"mr", "fmr", "mrr", "fmrr"} and all(got[k] == want[k] for k in want), (got, want)
    ranges, domains = build_type_constraints(c.train, c.R)
    per = [composed(desc, q, side, x.off.numpy(), x.ids.numpy(), c.E, q[:, 1], *((h_off, h_ids) if side else (t_off, t_ids)))
           for side, x in ((0, ranges), (1, domains))]
    want = cr.metrics(np.stack([per[1][0], per[0][0], per[1][1], per[0][1]]))
    got = ev.test_type_constrained(q, n)
    assert all(got[k] == want[k] for k in want), (got, want)
    a, b = ev.test_sampled(q, n, 50, seed=1), ev.test_sampled(q, n, 50, seed=1)
    assert a == b and a != ev.test_sampled(q, n, 50, seed=2) and a["mr"] <= 51


def test_debug_mode_checks_the_documented_preconditions():
    """The debug id mode refuses a skip segment that is not ascending, a list index and a triple id out of range; off, nothing is checked."""
    from pykg2vec_amd import _lib
    c, m = golden_model("transe_l1")
    desc = m.make_desc()
    d = hip_util.dev
    q = np.ascontiguousarray(c.test[:4], dtype=np.int64)
    off, ids = cr.csr_of([[1, 2, 3]] * 4)
    good = (d(np.asarray([0, 2, 2, 4, 5])), d(np.asarray([3, 7, 2, 2, 9]), torch.int32))        # ascending, equal ids allowed
    bad = (d(np.asarray([0, 2, 2, 4, 5])), d(np.asarray([3, 7, 5, 2, 9]), torch.int32))         # segment 2 descends at position 3
    call = lambda qq=q, loq=None, skip=good: K().rank_candidates(desc, d(qq), 0, d(off), d(ids, torch.int32), loq, skip[0], skip[1], skip_sorted=True)
    was = K().debug_enabled()
    K().set_debug(True)
    try:
        want = call().cpu().numpy()
        with pytest.raises(_lib.KgeHipError, match="ascending.*position 3"):
            call(skip=bad)
        with pytest.raises(_lib.KgeHipError, match="list_of_query"):
            call(loq=d(np.asarray([0, 1, 4, 0])))
        far = q.copy()
        far[2, 0] = c.E
        with pytest.raises(_lib.KgeHipError, match="head"):
            call(qq=far)
    finally:
        K().set_debug(was)
    assert np.array_equal(call().cpu().numpy(), want)
