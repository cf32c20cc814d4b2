"""CPU-only checks of triple classification: kge_classification_fit / _apply and kge_corrupt_typed refuse bad arguments before any GPU
call, the header's prototypes are what _lib binds, the numpy reference fit (tests/classification_ref.py) agrees with an independent
O(n^2) restatement that never looks at a key, and Evaluator.fit_thresholds / classify / test_classification plumb splits, negatives,
the global fallback, dropped rows and metrics correctly over an injected backend whose calls are that numpy reference."""
import ctypes
import math
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

import classification_ref as cr
import hip_util
import oracle_backend
import sampler_oracle as so
from golden_util import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _fit(lib, scores=FAKE, rel=FAKE, label=FAKE, n=4, R=3, higher=0, ws=FAKE, ws_bytes=1 << 20, thr=FAKE, fit=FAKE):
    return lib.kge_classification_fit(scores, rel, label, n, R, higher, ws, ws_bytes, thr, fit, None)


def _apply(lib, scores=FAKE, rel=FAKE, label=None, n=4, R=3, higher=0, thr=FAKE, seen=FAKE, thr_global=-1, pred=FAKE, conf=None):
    return lib.kge_classification_apply(scores, rel, label, n, R, higher, thr, seen, thr_global, pred, conf, None)


def _typed(lib, ph=FAKE, pr=FAKE, pt=FAKE, n=4, E=50, R=5, bern=None, off=FAKE, ids=FAKE, slots=None, n_slots=0, neg=FAKE, failed=FAKE):
    return lib.kge_corrupt_typed(ph, pr, pt, n, E, R, bern, off, ids, slots, n_slots, 1, 0, neg, failed, None)


@pytest.mark.parametrize("call, kw, word", [
    (_fit, dict(n=-1), b"n = -1"), (_fit, dict(n=(1 << 30) + 1), b"2^30"), (_fit, dict(R=0), b"R = 0"), (_fit, dict(R=1 << 20), b"2^20"),
    (_fit, dict(scores=None), b"scores"), (_fit, dict(rel=None), b"rel"), (_fit, dict(label=None), b"label"), (_fit, dict(thr=None), b"thr"),
    (_fit, dict(fit=None), b"fit"), (_fit, dict(ws=None), b"null workspace"), (_fit, dict(ws_bytes=16), b"workspace too small"),
    (_apply, dict(n=-1), b"n = -1"), (_apply, dict(R=1 << 20), b"2^20"), (_apply, dict(scores=None), b"scores"), (_apply, dict(rel=None), b"rel"),
    (_apply, dict(pred=None), b"pred"), (_apply, dict(thr=None), b"thr"), (_apply, dict(seen=None), b"seen"),
    (_apply, dict(label=FAKE), b"labels without conf"), (_apply, dict(thr_global=-2), b"thr_global"), (_apply, dict(thr_global=1 << 32), b"thr_global"),
    (_typed, dict(n=-1), b"n = -1"), (_typed, dict(E=1 << 24), b"2^24"), (_typed, dict(R=1 << 16), b"2^16"), (_typed, dict(ph=None), b"ph"),
    (_typed, dict(pr=None), b"pr"), (_typed, dict(pt=None), b"pt"), (_typed, dict(neg=None), b"neg"), (_typed, dict(off=None), b"type_off"),
    (_typed, dict(ids=None), b"type_ids"), (_typed, dict(failed=None), b"n_failed"), (_typed, dict(slots=FAKE, n_slots=24), b"power of two"),
    (_typed, dict(slots=FAKE, n_slots=8), b"power of two")])
def test_entry_points_refuse_bad_arguments_without_gpu(call, kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert call(lib, **kw) != 0
    who = {_fit: b"kge_classification_fit", _apply: b"kge_classification_apply", _typed: b"kge_corrupt_typed"}[call]
    assert word in lib.kge_last_error() and who in lib.kge_last_error(), lib.kge_last_error()


def test_workspace_grows_with_the_padded_sort_and_refused_sizes_are_zero():
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert [lib.kge_classification_sort_length(n) for n in (0, 1, 256, 257, 2048, 2049, 1 << 30)] == [256, 256, 256, 512, 2048, 4096, 1 << 30]
    assert lib.kge_classification_sort_length(-1) == 0 == lib.kge_classification_sort_length((1 << 30) + 1)
    for n, R in ((0, 1), (1, 1), (4097, 70), (100000, 1345)):
        need = lib.kge_classification_fit_workspace_bytes(n, R)
        lo = 8 * lib.kge_classification_sort_length(n) + 2 * 16 * max(1, -(-n // 1024)) + 40 * R
        assert lo <= need <= lo + 2048, (n, R, need, lo)
    assert lib.kge_classification_fit_workspace_bytes(-1, 1) == 0 == lib.kge_classification_fit_workspace_bytes(4, 1 << 20)
    assert lib.kge_classification_fit_workspace_bytes(4, 0) == 0


def test_header_prototypes_are_what_lib_binds():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_TYPED_ATTEMPTS\s+(\d+)", text).group(1)) == _lib.TYPED_ATTEMPTS == kernels.TYPED_ATTEMPTS == cr.TYPED_ATTEMPTS
    assert (int(re.search(r"#define\s+KGE_TYPED_UNIFORM_ATTEMPTS\s+(\d+)", text).group(1)) == _lib.TYPED_UNIFORM_ATTEMPTS
            == kernels.TYPED_UNIFORM_ATTEMPTS == cr.UNIFORM_ATTEMPTS)
    assert int(re.search(r"#define\s+KGE_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 3      # the entries are additive
    scalars = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}
    ctype_of = lambda arg: ctypes.c_void_p if "*" in arg else scalars[arg.split()[-2]]
    for name in ("kge_classification_sort_length", "kge_classification_fit_workspace_bytes", "kge_classification_fit", "kge_classification_apply",
                 "kge_corrupt_typed"):
        m = re.search(r"(\w+)\s+%s\(([^;]*)\);" % name, text)
        assert m, name
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
        res, bound = _lib._SIGNATURES[name]
        assert res is scalars[m.group(1)], name
        assert [ctype_of(a) for a in args] == list(bound), (name, args)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)


# ---------------------------------------------------------------------------------------------- the reference against a restatement
def _more_plausible(a, b, higher):
    """-1 / 0 / +1: a is more plausible than / as plausible as / less plausible than b, on the FLOATS (no key): a NaN is less plausible
    than every number and as plausible as another NaN; -0.0 == +0.0 by float comparison."""
    if math.isnan(a) or math.isnan(b):
        return 0 if math.isnan(a) and math.isnan(b) else (1 if math.isnan(a) else -1)
    if a == b:
        return 0
    return -1 if (a > b) == bool(higher) else 1


def _fit_quadratic(scores, rel, label, R, higher):
    """thr as a SCORE (None = nothing positive) + the fit row per relation, by pure double loops over the floats."""
    out = []
    for r in range(R):
        idx = [i for i in range(len(scores)) if rel[i] == r]
        s = [float(scores[i]) for i in idx]
        l = [bool(label[i]) for i in idx]
        cuts = []       # distinct number scores, most plausible first
        for c in s:
            if not math.isnan(c) and all(_more_plausible(c, d, higher) != 0 for d in cuts):
                cuts.append(c)
        for i in range(len(cuts)):          # insertion sort by plausibility: no sort key
            for j in range(i + 1, len(cuts)):
                if _more_plausible(cuts[j], cuts[i], higher) < 0:
                    cuts[i], cuts[j] = cuts[j], cuts[i]
        best, best_cut = sum(1 for x in l if not x), None
        for c in cuts:
            correct = 0
            for x, y in zip(s, l):
                pred = not math.isnan(x) and _more_plausible(x, c, higher) <= 0
                correct += pred == y
            if correct > best:
                best, best_cut = correct, c
        wins = ties = 0
        for x, y in zip(s, l):
            if not y:
                for x2, y2 in zip(s, l):
                    if y2:
                        c = _more_plausible(x2, x, higher)
                        wins, ties = wins + (c < 0), ties + (c == 0)
        out.append((best_cut, (sum(l), len(l) - sum(l), best, wins, ties, 0)))
    return out


def _random_case(rng, k):
    n = int(rng.integers(0, 40))
    R = int(rng.integers(1, 5))
    kind = k % 5
    if kind == 0:
        scores = rng.normal(size=n)
    elif kind == 1:
        scores = rng.integers(-2, 2, size=n).astype(np.float64)                 # four values: ties are the rule
    elif kind == 2:
        scores = np.full(n, 1.5)                                                 # every score equal
    else:
        scores = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45], dtype=np.float32), size=n)
    rel = rng.integers(0, R, size=n)
    if k % 7 == 0 and R > 1:
        rel[rel == R - 1] = 0                                                    # an empty relation
    label = rng.integers(0, 2, size=n)
    if k % 3 == 0:
        label[rel == 0] = 1                                                      # an all-positive relation
    if k % 3 == 1:
        label[rel == 0] = 0                                                      # an all-negative one
    return scores.astype(np.float32), rel.astype(np.int64), label.astype(np.uint8), R


def test_numpy_fit_agrees_with_the_quadratic_restatement_on_200_cases():
    rng = np.random.default_rng(11)
    seen_kinds = set()
    for k in range(200):
        scores, rel, label, R = _random_case(rng, k)
        higher = bool(k & 1)
        thr, rows = cr.fit(scores, rel, label, R, higher)
        want = _fit_quadratic(scores, rel, label, R, higher)
        for r in range(R):
            cut, row = want[r]
            assert tuple(rows[r]) == row, (k, r, rows[r], row)
            assert thr[r] == (-1 if cut is None else cr.keys_of([cut], higher)[0]), (k, r, thr[r], cut)
            seen_kinds.add(("none" if cut is None else "cut", row[0] == 0, row[1] == 0))
        # apply with the fitted thresholds reproduces the fit's own correct count
        pred, conf = cr.apply(scores, rel, thr, np.ones(R, np.uint8), -1, label, higher)
        assert np.array_equal(conf[:, 0] + conf[:, 2], rows[:, 2]) and np.array_equal(conf.sum(1), rows[:, 0] + rows[:, 1])
    assert {("none", True, True), ("none", True, False), ("cut", False, True), ("cut", False, False)} <= seen_kinds


def test_key_map_orders_floats_and_inverts():
    from pykg2vec_amd.evaluator import classification_key_to_score
    s = np.array([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.5, np.inf, np.nan], dtype=np.float32)
    lo, hi = cr.keys_of(s, False), cr.keys_of(s, True)
    assert lo[3] == lo[4] and hi[3] == hi[4] and lo[-1] == hi[-1] == cr.NAN_KEY
    assert (np.diff(np.delete(lo, 3)) > 0).all() and (np.diff(np.delete(hi, [3, 8])) < 0).all() and hi[:8].max() < cr.NAN_KEY
    for higher, k in ((False, lo), (True, hi)):
        back = classification_key_to_score(k[:8], higher)
        assert np.array_equal(back, np.where(s[:8] == 0, np.float32(0.0), s[:8])) and not np.signbit(back[3])
    assert np.isnan(classification_key_to_score([-1], False)[0])


def test_typed_draw_restatement_is_corrupt_one_when_every_entity_is_listed():
    """With the full entity range as every relation's list, ascending, a typed draw IS the uniform draw of oracle/sampler_oracle.py's
    corrupt_one (the same counter, key, side decision and multiply-shift), as long as that never redraws the replaced entity."""
    E, R, n = 37, 3, 200
    rng = np.random.default_rng(3)
    ph, pr, pt = rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)
    known = {(int(h), int(r), int(t)) for h, r, t in zip(ph, pr, pt)}
    off = np.stack([np.arange(R + 1) * E, (np.arange(R + 1) + R) * E]).astype(np.int64)
    ids = np.tile(np.arange(E, dtype=np.int32), 2 * R)
    neg, failed, fell = cr.corrupt_typed(ph, pr, pt, E, R, None, off, ids, known, 9, 100)
    assert failed == 0 and not fell.any()
    for i in range(n):
        assert tuple(neg[i]) == so.corrupt_one(int(ph[i]), int(pr[i]), int(pt[i]), E, 0.5, known, 9, 100 + i)


# ---------------------------------------------------------------------------------------------- plumbing over an injected backend
class Backend(types.SimpleNamespace):
    """oracle_backend + the classification calls as numpy restatements, with the calls recorded."""

    def __init__(self):
        super().__init__(**{k: v for k, v in vars(oracle_backend).items() if not k.startswith("__")})
        self.fits, self.applies, self.draws = [], [], []
        self.fail_rows = 0

    def classification_fit(self, scores, rel, label, n_relations, higher_is_better=False):
        self.fits.append((int(scores.numel()), int(n_relations)))
        return cr.classification_fit_torch(scores, rel, label, n_relations, higher_is_better)

    def classification_apply(self, scores, rel, thr, seen, thr_global, label=None, higher_is_better=False):
        self.applies.append((int(scores.numel()), label is not None))
        return cr.classification_apply_torch(scores, rel, thr, seen, thr_global, label, higher_is_better)

    def corrupt_typed(self, ph, pr, pt, E, R, bern, off, ids, slots, seed, offset):
        self.draws.append(("typed", int(ph.numel()), int(seed)))
        neg, failed = cr.corrupt_typed_torch(ph, pr, pt, E, R, bern, off, ids, slots, seed, offset)
        for i in range(self.fail_rows):      # rows the bounded redraw gave up on
            neg[3 * i + 1, 2] = -1
        return neg, failed + self.fail_rows

    def corrupt(self, ph, pr, pt, neg_rate, E, bern, slots, seed, offset):
        self.draws.append(("uniform", int(ph.numel()), int(seed)))
        return tuple(torch.from_numpy(a) for a in so.corrupt(ph.numpy(), pr.numpy(), pt.numpy(), neg_rate, E, bern, slots, seed, offset))


S = np.round(np.random.default_rng(5).normal(size=997) * 2).astype(np.float32)      # quantised scores: ties are the rule


def _score(trip):
    trip = np.asarray(trip)
    return S[(trip[:, 0] * 31 + trip[:, 1] * 7 + trip[:, 2] * 3) % 997]


def _setup(drop_relation=None):
    from pykg2vec_amd.evaluator import Evaluator
    c = Case("transe_l1")
    valid = c.valid if drop_relation is None else c.valid[c.valid[:, 1] != drop_relation]
    cfg = hip_util.make_config(c.E, c.R, c.hp, c.train, valid, c.test, device="cpu")
    m = hip_util.model_from_case(c, device="cpu")
    m.kernel_name = "ntn"
    St = torch.from_numpy(S)
    m.forward = lambda h, r, t: St[(h * 31 + r * 7 + t * 3) % 997]
    B = Backend()
    return c, cfg, m, Evaluator(m, cfg, backend=B), B, valid


def _reference(c, valid, test, seed_fit=0, seed_test=1, higher=False):
    known = {tuple(map(int, x)) for x in np.concatenate([c.train, valid, c.test])}
    off, ids = cr.type_lists(c.train, c.R)
    draw = lambda pos, seed: cr.corrupt_typed(pos[:, 0], pos[:, 1], pos[:, 2], c.E, c.R, None, off, ids, known, seed, 0)[0]
    lab = lambda pos: np.concatenate([np.ones(len(pos), np.uint8), np.zeros(len(pos), np.uint8)])
    both = np.concatenate([valid, draw(valid, seed_fit)])
    thr, rows = cr.fit(_score(both), both[:, 1], lab(valid), c.R, higher)
    gthr, grow = cr.fit(_score(both), np.zeros(len(both), np.int64), lab(valid), 1, higher)
    tb = np.concatenate([test, draw(test, seed_test)])
    seen = rows[:, 0] + rows[:, 1] > 0
    pred, conf = cr.apply(_score(tb), tb[:, 1], thr, seen, gthr[0], lab(test), higher)
    _, trow = cr.fit(_score(tb), tb[:, 1], lab(test), c.R, higher)
    return thr, rows, int(gthr[0]), grow[0], seen, pred, cr.metrics(conf, trow)


def test_default_splits_caching_and_metrics(capsys):
    c, cfg, m, ev, B, valid = _setup()
    thr, rows, gthr, grow, seen, pred, want = _reference(c, valid, c.test)
    got = ev.test_classification(epoch=4)                  # no thresholds yet: fitted on the validation split, seed 0; test split, seed 1
    out = capsys.readouterr().out
    assert "Triple Classification Results" in out and "Epoch: 4" in out and "accuracy" in out and "auc" in out
    assert B.draws == [("typed", len(valid), 0), ("typed", len(c.test), 1)]
    assert B.fits == [(2 * len(valid), c.R), (2 * len(valid), 1), (2 * len(c.test), c.R)] and B.applies == [(2 * len(c.test), True)]
    assert set(got) == {"accuracy", "accuracy_per_relation", "auc", "auc_per_relation", "confusion", "n_dropped"} and got["n_dropped"] == 0
    assert cr.same_metrics(got, want), (got, want)
    assert 0.0 <= got["auc"] <= 1.0 and got["confusion"].sum() == 2 * len(c.test)
    th = ev.thresholds
    assert np.array_equal(th.key, thr) and np.array_equal(th.fit, rows) and th.global_key == gthr and np.array_equal(th.global_fit, grow)
    assert np.array_equal(th.seen, seen) and th.key.dtype == np.int64 and th.value.dtype == np.float32 and not th.higher_is_better
    assert np.array_equal(cr.keys_of(th.value[thr >= 0], False), thr[thr >= 0]) and np.isnan(th.value[thr < 0]).all()
    # the stored thresholds are reused: a second test fits only the test scores' AUC
    B.fits.clear()
    again = ev.test_classification(c.test, 20)
    assert B.fits == [(40, c.R)] and cr.same_metrics(again, _reference(c, valid, c.test[:20])[6])
    # classify: the apply step without labels, on the same thresholds
    tb = np.concatenate([c.test, c.test[:, ::-1]])
    flags = ev.classify(tb)
    assert flags.dtype == torch.bool and np.array_equal(flags.numpy(), cr.apply(_score(tb), tb[:, 1], thr, seen, gthr, None, False)[0] != 0)
    assert B.applies[-1] == (len(tb), False)
    # given negatives are used as they are; their number must match
    neg = c.test[::-1].copy()
    given = ev.test_classification(c.test, None, negatives=neg)
    tb = np.concatenate([c.test, neg])
    lab = np.concatenate([np.ones(len(neg), np.uint8), np.zeros(len(neg), np.uint8)])
    _, conf = cr.apply(_score(tb), tb[:, 1], thr, seen, gthr, lab, False)
    assert np.array_equal(given["confusion"], conf) and len(B.draws) == 3       # nothing more was drawn
    with pytest.raises(ValueError, match="one negative per positive"):
        ev.test_classification(c.test, None, negatives=neg[:5])


def test_higher_is_better_flips_the_orientation_and_uniform_negatives_use_the_training_sampler():
    c, cfg, m, ev, B, valid = _setup()
    m.higher_is_better = True
    thr, rows, gthr, grow, seen, pred, want = _reference(c, valid, c.test, higher=True)
    got = ev.test_classification()
    assert cr.same_metrics(got, want) and ev.thresholds.higher_is_better
    assert np.array_equal(cr.keys_of(ev.thresholds.value[thr >= 0], True), thr[thr >= 0])
    neg = ev.classification_negatives(c.test, 30, seed=5, typed=False)
    assert B.draws[-1] == ("uniform", 30, 5) and tuple(neg.shape) == (30, 3) and neg.dtype == torch.int64
    known = {tuple(map(int, x)) for x in np.concatenate([c.train, valid, c.test])}
    nh, nr, nt = so.corrupt(c.test[:30, 0], c.test[:30, 1], c.test[:30, 2], 1, c.E, None, known, 5, 0)
    assert np.array_equal(neg.numpy(), np.stack([nh, nr, nt], 1)) and not any(tuple(map(int, x)) in known for x in neg.numpy())


def test_relation_without_validation_triples_falls_back_to_the_global_threshold():
    c, cfg, m, ev, B, valid = _setup(drop_relation=1)
    assert (c.test[:, 1] == 1).any() and not (valid[:, 1] == 1).any()
    thr, rows, gthr, grow, seen, pred, want = _reference(c, valid, c.test)
    assert not seen[1] and thr[1] == -1 and gthr >= 0
    got = ev.test_classification()
    assert cr.same_metrics(got, want) and not ev.thresholds.seen[1] and ev.thresholds.global_key == gthr
    assert got["confusion"][1, 0] + got["confusion"][1, 1] > 0      # the relation's triples ARE classified positive somewhere: not by thr = -1
    assert cr.keys_of([ev.thresholds.global_value], False)[0] == gthr


def test_dropped_rows_leave_with_their_positive_and_more_than_one_percent_is_an_error(capsys):
    c, cfg, m, ev, B, valid = _setup()
    data = np.concatenate([c.test] * (1 + 300 // len(c.test)))[:300]
    ev.fit_thresholds()       # on the small validation split, before any draw fails
    B.fail_rows = 2
    neg = ev.classification_negatives(data, 300, seed=3)
    assert "dropped 2 of 300" in capsys.readouterr().out and ev.n_dropped == 2 and tuple(neg.shape) == (298, 3) and (neg.numpy() >= 0).all()
    pos, neg2, dropped = ev._labelled_pairs(data, 300, None, 3)
    keep = np.ones(300, bool)
    keep[[1, 4]] = False
    assert dropped == 2 and np.array_equal(pos.numpy(), data[keep]) and np.array_equal(neg2.numpy(), neg.numpy())
    assert (pos[:, 1] == neg2[:, 1]).all() and ((pos[:, 0] == neg2[:, 0]) | (pos[:, 2] == neg2[:, 2])).all()      # still paired row by row
    got = ev.test_classification(data, 300, seed=3)
    assert got["n_dropped"] == 2 and got["confusion"].sum() == 2 * 298
    B.fail_rows = 4
    from pykg2vec_amd._lib import KgeHipError
    with pytest.raises(KgeHipError, match="bounded redraw"):
        ev.classification_negatives(data, 300, seed=3)


def test_thresholds_pickle_to_plain_numpy_and_metric_arithmetic():
    from pykg2vec_amd.evaluator import ClassificationThresholds, classification_metrics
    c, cfg, m, ev, B, valid = _setup()
    th = ev.fit_thresholds()
    assert th is ev.thresholds
    back = pickle.loads(pickle.dumps(th))
    for name in ("key", "value", "seen", "fit", "global_fit"):
        assert type(getattr(back, name)) is np.ndarray and np.array_equal(getattr(back, name), getattr(th, name), equal_nan=name == "value")
    assert back.global_key == th.global_key and back.higher_is_better == th.higher_is_better
    assert np.array_equal(ev.classify(c.test[:9], thresholds=back).numpy(), ev.classify(c.test[:9]).numpy())
    conf = np.array([[3, 1, 2, 0], [0, 0, 0, 0], [1, 1, 1, 1]])
    rows = np.array([[3, 3, 0, 7, 2, 0], [0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0]])
    got = classification_metrics(conf, rows)
    assert got["accuracy"] == 7 / 10 and got["auc"] == 8 / 9
    assert np.array_equal(got["accuracy_per_relation"], [5 / 6, np.nan, 0.5], equal_nan=True)
    assert np.array_equal(got["auc_per_relation"], [8 / 9, np.nan, np.nan], equal_nan=True) and cr.same_metrics(got, cr.metrics(conf, rows))
    t2 = ClassificationThresholds([-1, 5], np.zeros((2, 6), np.int64), -1, np.zeros(6, np.int64), False)
    assert np.isnan(t2.value[0]) and np.isnan(t2.global_value) and not t2.seen.any()
