"""Every training-step path and the optimiser row kernels at the hidden sizes where their geometry switches, against float64.

The training kernels choose a register or float4 geometry from the hidden size d; each choice has a threshold at which it switches to
another kernel, another lane-group width, a float4 or dword row layout, or falls through to another step path.  An off-by-one there
(`<=` for `<`, `nvec` for `dim`) corrupts or drops the last float4 of every row at exactly one hidden size, and a fall-through that
silently changes path goes equally unnoticed.  The thresholds, as the sources state them (THRESHOLDS below cites the lines):

    generic "push" step / forward   pick_geometry: (32,1) <= 32, (32,2) <= 64, (32,4) <= 128, (32,8) <= 256, (64,8) <= 512,
                                    (64,16) <= 1024, (64,32) <= 2048, wider refused
    pull   (TransE, TransM)         d % 4 == 0, d <= 1024; NV = 1 / 2 / 4 / 8 at d / 4 <= 32 NV; KGE_PULL_G=16: NV 1 / 2 at d / 4 <= 16 / 32
    own    (DistMult, ComplEx)      float4 rows: (32,1) d / 4 <= 32, (64,1) <= 64, (64,2) up to 512; Trainer admits d % 4 == 0 only
    ownx   (ANALOGY, CP, SimplE, SimplE_ignr, QuatE)   pick_geometry up to d = 256 (dword rows), ANALOGY even d only
    transx (TransH, TransD)         d % 4 == 0, d <= 512; NV = 1 / 2 / 4 at d / 4 <= 32 / 64
    staged (RotatE)                 d % 4 == 0, d <= 2048; pick_geometry for the bundle kernel (four waves per bundle above 1024),
                                    k_opt_staged NV = 1 / 2 / 4 / 8 at d / 4 <= 64 / 128 / 256 / 512
    optimiser rows                  k_opt_rows4<NV> at d <= 128 NV (d % 4 == 0, d <= 1024, 16-byte aligned buffers), else k_opt_rows<NCH>
                                    at d <= 64 NCH, NCH 4 / 8 / 16; eight rows per block in the float4 form, four in the dword form

Part 1 (one step per path and width): the method and the bar of tests/test_hip_skew.py (tests/step_bar.py): Trainer(use_graph=False),
one SGD step with lr = 1 through train_model_epoch(0), so that before - after is the step's gradient; the batch restated by
K.sample_batch on the same counters; the float64 oracle's gradient of that batch; per element
    2e-6 + 2e-4 |g64| + c_r 2^-23 a_r + 2^-24 |after| (+ the near-margin / near-zero allowance; ambiguous pairs <= 1 % of pairs),
the loss at rtol 2e-5, forward() on the batch's positives at atol = rtol = 2e-5.  Shapes: E = 40, R = 5 (2 where a table is k x k or
larger), B = 64, a train split of three batches and 17 more rows; uniform ids then give every row several incidences.  Every case
first asserts the step path the Trainer reports, which pins the fall-through widths.  The atomic-free paths run twice and must
reproduce the flat parameter buffer bit for bit.  The generic "push" step is run as tests/test_hip_edges.py runs it: eager, no
switch, on an explicit batch (the oracle batch and its first 37 pairs, ragged against 8 groups per workgroup), its gradient read
from the flat gradient buffer (so the bar's |after| term is absent).

With 64 pairs the 1 % cap allows no ambiguous pair at all.  An L1 residual component within 1e-6 of zero is expected once per
~60 000 components, so the wide L1 cases draw their tables from the first seed (SEEDS, searched on the float64 oracle alone) whose
batch has none; test_reference_fp32_meets_the_bar checks every case's inputs and bar on the CPU against the fp32 numpy oracle before
any GPU time is spent, with the batch from oracle/sampler_oracle.py, which the GPU cases assert K.sample_batch reproduces.

TransH / TransD / TransR run with the L2 norm here (as tests/test_hip_skew.py does for TransH): the near-zero allowance is derived
for the TransE / TransM residual only.

Part 1c (optimiser state at the edges): three Adam / Adagrad steps on each owner path at one width below and at each threshold,
against three float64 oracle steps; atol = rtol = 1e-4 (tests/test_hip_own.py::test_three_own_steps_match_reference_weights); an element
may miss that only where its float64 gradient is below NEAR_ZERO in one of the steps (Adam's first step is sign-like), and the elements
so excluded are at most 0.2 % of the touched ones (the allowance of test_own_epochs_equal_push_epochs, which counts the elements
that miss its tolerance).

Part 2 (optimiser row kernels): K.optimizer_step_rows against the flat K.optimizer_step on identical buffers, bit for bit, and the
flat form against float64.

Part 1d: the dword form of own_geo (csrc/kge_own.hip:595-599: (32,4) d <= 128, (64,4) <= 256, (64,8) <= 512 for d % 4 != 0) is never
selected by Trainer._own_ok, which admits d % 4 == 0 only; Trainer.own_step_explicit (K.own_step + K.own_apply on an explicit batch)
reaches it, and it is held to the same bar there.  No geometry of the tables above was found to be unreachable."""
import collections
import functools
import zlib

import numpy as np
import pytest

import kge_oracle as ko
import sampler_oracle as so
import step_bar as sb

gpu = pytest.mark.gpu

E, B = 40, 64
N_TRAIN = 3 * B + 17
RAGGED = 37            # ragged against 8 groups per workgroup (tests/test_hip_edges.py)
GEN_SEED = 0           # hip_util.make_config: seed = 0
SWITCHES = ("KGE_PULL", "KGE_PULL_DIR", "KGE_PULL_G", "KGE_PW_PULL", "KGE_STAGED", "KGE_TRANSX_OWN", "KGE_OWN_STAGED", "KGE_RESCAL_FUSED",
            "KGE_RESCAL_UNFUSED", "KGE_RESCAL_STAGED", "KGE_GRAPH_MULTI", "KGE_OPT_RIDER", "KGE_NTN_BIG", "KGE_OPT_NT")

# The thresholds T of each path's own table, copied from the sources (never from a kernel's results).  (path, T, step s, source)
THRESHOLDS = [
    ("generic", (32, 64, 128, 256, 512, 1024, 2048), 1, "csrc/kge_api.hip:23-34 pick_geometry"),
    ("pull", (128, 256, 512, 1024), 4, "csrc/kge_pull.hip:718-731 pull_geo: nvec <= 32 * nv, nv = 1, 2, 4, 8; dim > 1024 refused"),
    ("pull_g16", (64, 128), 4, "csrc/kge_pull.hip:722-724 pull_geo, KGE_PULL_G=16: nvec <= 16 -> NV 1, nvec <= 32 -> NV 2"),
    ("own", (128, 256, 512), 4, "csrc/kge_own.hip:584-594 own_geo: nvec <= 32, nvec <= 64, dim <= 512; trainer.py:477 d % 4 == 0"),
    ("own_dword", (128, 256, 512), 1, "csrc/kge_own.hip:595-599 own_geo, d % 4 != 0: dim <= 128, dim <= 256, dim <= 512"),
    ("ownx", (32, 64, 128, 256), 1, "csrc/kge_ownx.hip:312-315 ownx_geo: pick_geometry, dim <= 256, ANALOGY even"),
    ("transx", (128, 256, 512), 4, "csrc/kge_pullx.hip:387-390: dim % 4, dim <= 512, NV by nvec <= 32 / 64; trainer.py:581"),
    ("staged", (256, 1024, 2048), 4, "csrc/kge_staged.hip:290-293 k_opt_staged NV by nvec <= 64 / 128 / 256 / 512; pick_geometry; "
                                     "trainer.py:642 d % 4 == 0, d <= 2048"),
    ("opt_rows4", (128, 256, 512, 1024), 4, "csrc/kge_opt.hip:324-326 rows4_ok, :353-361 dim <= 128 * NV"),
    ("opt_rows", (256, 512, 1024), 1, "csrc/kge_opt.hip:372-378 dim <= 64 * NCH, NCH 4 / 8 / 16; csrc/kge_api.hip:459 dim <= 1024"),
]

Case = collections.namedtuple("Case", "key group model hp env path R neg pointwise refused")
CASES = {}


def _add(group, model, hp, env, path, tag="", R=5, refused=None):
    neg = int(hp.get("neg_rate", 1))
    widths = "x".join(str(hp[k]) for k in ("hidden_size", "ent_hidden_size", "rel_hidden_size") if k in hp)
    key = "%s/%s%s/d%s" % (group, model, tag, widths)
    assert key not in CASES, key
    CASES[key] = Case(key, group, model, hp, env, path, R, neg, model in ko.POINTWISE, refused)


def _straddle(thresholds, s, lo, hi=None, outside=()):
    out = {lo}
    for t in thresholds:
        out.update((t - s, t, t + s))
    if hi is not None:
        out = {w for w in out if w <= hi} | {hi}
    return sorted(w for w in out if w >= lo), list(outside)


# ---- pull: TransE L1 / L2, TransM (csrc/kge_pull.hip)
PULL_W = [4, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1020, 1024]
assert PULL_W == _straddle(dict((t[0], t[1]) for t in THRESHOLDS)["pull"], 4, 4, 1024)[0]
for model, l1, tag in (("transe", True, "_l1"), ("transe", False, "_l2"), ("transm", True, "_l1")):
    for d in PULL_W:
        _add("pull", model, dict(hidden_size=d, l1_flag=l1, margin=1.0), {"KGE_PULL": "1"}, "pull", tag)
    for d in (1028, 130):      # beyond the domain / no row of float4s: Trainer._pull_shape_ok refuses, the atomic step serves
        _add("pull", model, dict(hidden_size=d, l1_flag=l1, margin=1.0), {"KGE_PULL": "1"}, "generic", tag)
    for d in (60, 64, 68, 124, 128, 132):
        _add("pull_g16", model, dict(hidden_size=d, l1_flag=l1, margin=1.0), {"KGE_PULL": "1", "KGE_PULL_G": "16"}, "pull", tag)
for d in (128, 256, 512, 1024):    # the L1 two-phase form (Trainer.PULL_TWO_PHASE_MIN_BATCH), forced as tests/test_hip_pull.py forces it
    _add("pull_two_phase", "transe", dict(hidden_size=d, l1_flag=True, margin=1.0), {"KGE_PULL": "1", "KGE_PULL_DIR": "1"}, "pull", "_l1")

# ---- own: DistMult, ComplEx (csrc/kge_own.hip)
OWN_W = [4, 124, 128, 132, 252, 256, 260, 508, 512]
assert OWN_W == _straddle(dict((t[0], t[1]) for t in THRESHOLDS)["own"], 4, 4, 512)[0]
for model in ("distmult", "complex"):
    for d in OWN_W:
        _add("own", model, dict(hidden_size=d, lmbda=1e-3, neg_rate=1), {"KGE_PW_PULL": "1"}, "own")
    for d in (516, 130):
        _add("own", model, dict(hidden_size=d, lmbda=1e-3, neg_rate=1), {"KGE_PW_PULL": "1"}, "generic")

# ---- own, dword rows (d % 4 != 0): reached through Trainer.own_step_explicit only
for model in ("distmult", "complex"):
    for d in (1, 3, 126, 127, 129, 130, 254, 255, 257, 258, 510, 511):
        _add("own_dword", model, dict(hidden_size=d, lmbda=1e-3, neg_rate=1), {}, "explicit")

# ---- ownx: the model-generic staged owner step (csrc/kge_ownx.hip); dword rows, so s = 1 (ANALOGY: even sizes, s = 2)
OWNX_W = sorted(set([4, 124, 128, 132, 252, 256] + _straddle(dict((t[0], t[1]) for t in THRESHOLDS)["ownx"], 1, 1, 256)[0]))
OWNX_W_EVEN = sorted(set([4, 124, 128, 132, 252, 256] + [w for w in _straddle(dict((t[0], t[1]) for t in THRESHOLDS)["ownx"], 2, 2, 256)[0]]))
for model in ("analogy", "cp", "simple", "simple_ignr", "quate"):
    for d in (OWNX_W_EVEN if model == "analogy" else OWNX_W):
        _add("ownx", model, dict(hidden_size=d, lmbda=1e-3, neg_rate=1), {"KGE_PW_PULL": "1"}, "own")
    for d in ((258, 260) if model == "analogy" else (257, 260)):
        _add("ownx", model, dict(hidden_size=d, lmbda=1e-3, neg_rate=1), {"KGE_PW_PULL": "1"}, "generic")

# ANALOGY with an odd size: ownx_geo refuses it, the generic step is reported, and the library refuses the model (csrc/kge_api.hip:60)
_add("ownx", "analogy", dict(hidden_size=33, lmbda=1e-3, neg_rate=1), {"KGE_PW_PULL": "1"}, "generic", refused="even hidden size")

# ---- transx: TransH, TransD (csrc/kge_pullx.hip)
TRANSX_W = [4, 124, 128, 132, 252, 256, 260, 508, 512]
for d in TRANSX_W + [516]:
    path = "transx" if d <= 512 else "generic"
    _add("transx", "transh", dict(hidden_size=d, l1_flag=False, margin=1.0), {"KGE_TRANSX_OWN": "1"}, path)
    _add("transx", "transd", dict(ent_hidden_size=d, rel_hidden_size=d, l1_flag=False, margin=1.0), {"KGE_TRANSX_OWN": "1"}, path)
# TransD with unequal sizes: the owner path's predicate asks for one row length, and the library refuses the model outright
# (csrc/kge_api.hip:56-59: the reference's forward broadcasts the two, pairwise.py:277-278)
_add("transx", "transd", dict(ent_hidden_size=128, rel_hidden_size=64, l1_flag=False, margin=1.0), {"KGE_TRANSX_OWN": "1"}, "generic",
     refused="ent_hidden_size == rel_hidden_size")

# ---- staged: RotatE, neg_rate 2 (csrc/kge_staged.hip)
STAGED_W = [4, 252, 256, 260, 1020, 1024, 1028, 2044, 2048]
for d in STAGED_W:
    _add("staged", "rotate", dict(hidden_size=d, margin=6.0, neg_rate=2, alpha=0.5), {"KGE_STAGED": "1"}, "staged")
# 2052: Trainer._staged_ok refuses (d <= 2048), the generic step is reported, and its kernels refuse the row length loudly
_add("staged", "rotate", dict(hidden_size=2052, margin=6.0, neg_rate=2, alpha=0.5), {"KGE_STAGED": "1"}, "generic", refused="exceeds")

# ---- generic: the eager, unforced push step of all sixteen oracle models
GENERIC_W = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]
GENERIC_W_EVEN = [2, 30, 32, 34, 62, 64, 66, 126, 128, 130, 254, 256, 258, 510, 512, 514, 1022, 1024, 1026, 2046, 2048]


def _generic_hp(model, d, d2=None):
    if model in ("transe", "transm"):
        return dict(hidden_size=d, l1_flag=bool(d % 2), margin=1.0)
    if model == "transh":
        return dict(hidden_size=d, l1_flag=False, margin=1.0)
    if model == "transd":
        return dict(ent_hidden_size=d, rel_hidden_size=d, l1_flag=False, margin=1.0)
    if model == "transr":
        return dict(ent_hidden_size=d, rel_hidden_size=d2, l1_flag=False, margin=1.0)
    if model == "rotate":
        return dict(hidden_size=d, margin=6.0, neg_rate=2, alpha=0.5)
    if model == "rescal":
        return dict(hidden_size=d, margin=1.0, neg_rate=1)
    if model == "ntn":
        return dict(ent_hidden_size=d, rel_hidden_size=d2, lmbda=0.1, margin=1.0)
    return dict(hidden_size=d, lmbda=1e-3, neg_rate=1)


for model in ko.PAIRWISE + ko.POINTWISE:
    if model in ("rescal", "ntn", "transr"):
        continue
    for d in (GENERIC_W_EVEN if model == "analogy" else GENERIC_W):
        _add("generic", model, _generic_hp(model, d), {}, "generic")
# RESCAL: k <= 512 (csrc/kge_dense.hip:475); the pair form takes even k <= 256 and k % 4 rows as float4 (csrc/kge_api.hip:422-423)
for k in sorted(set([w for w in GENERIC_W if w <= 512] + [2, 6, 254, 256, 258])):
    _add("generic", "rescal", _generic_hp("rescal", k), {}, "generic", R=2)
_add("generic", "rescal", _generic_hp("rescal", 513), {}, "generic", R=2, refused="exceeds")
# NTN: ent_hidden_size <= 256, rel_hidden_size <= 1024 (csrc/kge_ntn.hip:811); each width straddled with the other interior
for d in [w for w in GENERIC_W if w <= 256]:
    _add("generic", "ntn", _generic_hp("ntn", d, 4), {}, "generic", R=2)
for kr in [w for w in GENERIC_W if w <= 1024]:
    _add("generic", "ntn", _generic_hp("ntn", 12, kr), {}, "generic", R=2)
_add("generic", "ntn", _generic_hp("ntn", 257, 4), {}, "generic", R=2, refused="ent_hidden_size <= 256")
# TransR: <= 128 per side (csrc/kge_transr.hip:24, :274)
for d in [w for w in GENERIC_W if w <= 128]:
    _add("generic", "transr", _generic_hp("transr", d, 24), {}, "generic")
    if d != 24:
        _add("generic", "transr", _generic_hp("transr", 24, d), {}, "generic")
_add("generic", "transr", _generic_hp("transr", 129, 24), {}, "generic", refused="exceed")

# Table seeds (second word of the world's seed) of the cases whose seed-0 batch holds an ambiguous pair in float64: the first seed
# without one, found by `PYTHONPATH=oracle:tests python tests/test_hip_width_edges.py` on the oracle alone and checked by test_reference_fp32_meets_the_bar.
SEEDS = {'pull/transe_l1/d128': 1, 'pull/transe_l1/d260': 1, 'pull/transe_l1/d508': 2, 'pull/transe_l1/d516': 2, 'pull/transe_l1/d1024': 13,
         'pull/transm_l1/d508': 1, 'pull/transm_l1/d512': 1, 'pull/transm_l1/d1024': 3, 'pull/transm_l1/d1028': 5,
         'pull_two_phase/transe_l1/d128': 1, 'generic/transe/d511': 1, 'generic/transe/d513': 3, 'generic/transe/d1023': 3,
         'generic/transe/d1025': 7, 'generic/transe/d2047': 2, 'generic/transm/d511': 1, 'generic/transm/d513': 1,
         'generic/transm/d1023': 2, 'generic/transm/d2047': 103}

OWNER_GROUPS = ("pull", "pull_g16", "pull_two_phase", "own", "ownx", "transx", "staged")
STEP_KEYS = [k for k, c in CASES.items() if c.group in OWNER_GROUPS]
GENERIC_KEYS = [k for k, c in CASES.items() if c.group == "generic"]


# ------------------------------------------------------------------------------------------------------ inputs and references
def _perm(train):
    """The batch order of pykg2vec_amd.generator.Generator (seed GEN_SEED, batch size B): one permutation, each batch slice ordered by
    relation id."""
    perm = np.random.default_rng(GEN_SEED).permutation(len(train))
    for lo in range(0, len(train), B):
        sl = perm[lo:lo + B]
        perm[lo:lo + B] = sl[np.argsort(train[sl, 1], kind="stable")]
    return perm


def oracle_batch(train, step, neg, pointwise):
    """Batch `step` of the epoch as oracle/sampler_oracle.py restates the device sampler (Philox counter offset = draws so far)."""
    pos = train[_perm(train)[step * B:(step + 1) * B]]
    train_set = {tuple(map(int, x)) for x in train}
    nh, nr, nt = so.corrupt(pos[:, 0], pos[:, 1], pos[:, 2], neg, E, None, train_set, GEN_SEED, step * B * neg)
    if pointwise:
        return tuple(np.asarray(x) for x in ko.pointwise_layout(pos, nh, nr, nt, neg))
    return (pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), nh, nr, nt)


def ragged(c, batch):
    """The first RAGGED pairs (bundles) of a batch."""
    if c.pointwise:
        return tuple(x[:RAGGED * (1 + c.neg)] for x in batch)
    return tuple(x[:RAGGED] for x in batch[:3]) + tuple(x[:RAGGED * c.neg] for x in batch[3:])


def _shape_kw(c):
    kw = {k: v for k, v in c.hp.items() if k in ("hidden_size", "ent_hidden_size", "rel_hidden_size")}
    if c.model == "rotate":
        kw["margin"] = c.hp["margin"]
    return kw


@functools.lru_cache(maxsize=None)
def train_split(R):
    rng = np.random.default_rng(1000 + R)
    return np.stack([rng.integers(E, size=N_TRAIN), rng.integers(R, size=N_TRAIN), rng.integers(E, size=N_TRAIN)], 1).astype(np.int64)


def world(key, table_seed=None):
    """(train split, tables, the oracle's hyper-parameters) of a case."""
    c = CASES[key]
    train = train_split(c.R)
    seed = SEEDS.get(key, 0) if table_seed is None else table_seed
    P = ko.init_params(c.model, np.random.default_rng((zlib.crc32(key.encode()), seed)), tot_entity=E, tot_relation=c.R, **_shape_kw(c))
    ohp = dict(c.hp)
    if c.model == "transm":
        ohp["theta"] = ko.transm_theta(train, c.R)
    return train, P, ohp


def quick_ambiguous(c, P, batch, ohp):
    """Pairs of the batch that fp32 and float64 may decide differently (step_bar.ambiguity_allowance counts the same), cheaply."""
    if c.model not in sb.HINGE:
        return 0
    ph, pr, pt, nh, nr, nt = batch
    Pn = ko.rescal_normalize_tables(P, np.float64) if c.model == "rescal" else P
    pos = ko.score(c.model, Pn, ph, pr, pt, dtype=np.float64, **ohp)
    neg = ko.score(c.model, Pn, nh, nr, nt, dtype=np.float64, **ohp)
    v = pos + float(ohp["margin"]) - neg
    amb = np.abs(v) < sb.NEAR_MARGIN
    if c.model in ("transe", "transm") and ohp.get("l1_flag"):
        for h, r, t in ((ph, pr, pt), (nh, nr, nt)):
            u = sb._l1_residual(P, h, r, t)[1][6]
            amb |= (np.abs(u) < sb.NEAR_ZERO).any(1) & (v > 0)
    return int(amb.sum())


Ref = collections.namedtuple("Ref", "batch loss G64 scores cnt a allow n_amb n_pairs")


def _reference_of(c, P, ohp, batch):
    G64, scores, cnt, side_of, a, ctx = sb.hub_bounds(c.model, P, batch, ohp, E, c.R)
    allow, n_amb = sb.ambiguity_allowance(c.model, P, scores, batch, ohp, ctx)
    widen = sb.normalisation_allowance(c.model, ko.rescal_normalize_tables(P, np.float64) if c.model == "rescal" else P, batch, ohp)
    allow = {k: v + widen[k] for k, v in allow.items()}      # (derived in step_bar.normalisation_allowance; zero but for normalised vectors of length 1)
    loss = float(ko.train_step_grads(c.model, P, batch, dtype=np.float64, **ohp)[0])
    n_pairs = len(batch[3]) if c.model == "rotate" else len(batch[0])      # (pairs; scored rows of the pointwise models)
    return Ref(batch, loss, G64, scores, cnt, a, allow, n_amb, n_pairs)


@functools.lru_cache(maxsize=64)
def reference(key, short=False):
    """The float64 side of a case's first batch (or of its first RAGGED pairs): gradient, scores, loss and the bar's terms."""
    c = CASES[key]
    train, P, ohp = world(key)
    batch = oracle_batch(train, 0, c.neg, c.pointwise)
    return _reference_of(c, P, ohp, ragged(c, batch) if short else batch)


def compare(key, ref, got, after=None):
    """Hold `got` (per-table gradients) to the bar; -> (largest deviation, largest deviation / tolerance)."""
    assert ref.n_amb <= 0.01 * ref.n_pairs, (key, ref.n_amb, ref.n_pairs)
    worst, ratio = 0.0, 0.0
    for k, g in ref.G64.items():
        tol = sb.tolerance(g, ref.cnt[k], ref.a[k], None if after is None else after[k], ref.allow[k])
        err = np.abs(np.asarray(got[k], np.float64) - g)
        bad = err > tol
        if bad.any():
            rows = np.flatnonzero(bad.reshape(len(g), -1).any(1))
            i = np.unravel_index(np.argmax(np.where(bad, err / tol, 0)), g.shape)
            raise AssertionError("%s %s: %d rows off (first %s); worst %s: got %.9g want %.9g tol %.3g c_r %d a_r %.4g"
                                 % (key, k, len(rows), rows[:8].tolist(), i, np.asarray(got[k])[i], g[i], tol[i], ref.cnt[k][i[0]], ref.a[k][i]))
        worst, ratio = max(worst, float(err.max())), max(ratio, float((err / tol).max()))
    return worst, ratio


# ------------------------------------------------------------------------------------------------------ 1e: CPU pre-check
def test_case_table_covers_every_threshold():
    """Every threshold T of a path's table is met at T - s, T and T + s (or the path's fall-through), with the smallest and the
    largest legal width, and every case names the path the sources give it."""
    widths = lambda group, model: sorted({c.hp.get("hidden_size", c.hp.get("ent_hidden_size")) for c in CASES.values()
                                          if c.group == group and c.model == model})
    for path, ts, s, _src in THRESHOLDS:
        group = {"opt_rows4": None, "opt_rows": None, "own_dword": None}.get(path, path)
        if group is None:      # (the optimiser widths are lists of their own; the dword own form takes T - 1 and T + 1 only: T % 4 == 0)
            continue
        models = sorted({c.model for c in CASES.values() if c.group == group})
        assert models, path
        for model in models:
            have = widths(group, model)
            step = 2 if (model == "analogy" and s == 1) else s
            limit = {"transr": 128, "ntn": 256, "rescal": 512}.get(model, 10 ** 9)
            for t in ts:
                for w in (t - step, t, t + step):
                    if w <= limit + step and not (group == "generic" and w > 2048):
                        assert w in have, (path, model, w)
    for c in CASES.values():
        d = c.hp.get("hidden_size", c.hp.get("ent_hidden_size"))
        if c.group in ("pull", "pull_g16", "pull_two_phase"):
            assert (c.path == "pull") == (d % 4 == 0 and d <= 1024), c.key
        elif c.group == "own":
            assert (c.path == "own") == (d % 4 == 0 and d <= 512), c.key
        elif c.group == "ownx":
            assert (c.path == "own") == (d <= 256 and not (c.model == "analogy" and d % 2)), c.key
        elif c.group == "transx":
            assert (c.path == "transx") == (d % 4 == 0 and d <= 512 and c.hp.get("rel_hidden_size", d) == d), c.key
        elif c.group == "staged":
            assert (c.path == "staged") == (d % 4 == 0 and d <= 2048), c.key


def test_library_geometry_agrees_with_the_case_table():
    """The library's own geometry queries (host code: no GPU needed) admit exactly the widths the case table sends down an owner path."""
    from pykg2vec_amd import kernels as K
    for c in CASES.values():
        d = c.hp.get("hidden_size", c.hp.get("ent_hidden_size"))
        if c.group in ("pull", "pull_two_phase"):
            assert (K.pull_groups_per_block(d) > 0) == (c.path == "pull"), c.key
        elif c.group in ("own", "ownx"):
            # (own_geo also admits d % 4 != 0 -- its dword form; the Trainer does not: those widths report "generic")
            assert (K.own_groups_per_block(c.model, d) > 0) == (c.path == "own" or (c.group == "own" and d <= 512)), c.key
        elif c.group == "transx" and c.hp.get("rel_hidden_size", d) == d:
            assert (K.transx_groups_per_block(d) > 0) == (c.path == "transx"), c.key
        elif c.group == "own_dword":
            assert K.own_groups_per_block(c.model, d) == (8 if d <= 128 else 4) and d % 4, c.key
    # groups per workgroup halve where the lane group doubles (own: nvec 32 -> 33), and the partial-sum row grows with NV
    assert [K.own_groups_per_block("complex", d) for d in (124, 128, 132)] == [8, 8, 4]
    assert [K.pull_partial_stride(d) for d in (124, 128, 132, 256, 260, 512, 516, 1024)] == [128, 128, 256, 256, 512, 512, 1024, 1024]
    assert [K.transx_partial_stride(d) > 0 for d in (128, 132, 256, 260, 512)] == [True] * 5


@pytest.mark.parametrize("key", [k for k in CASES if CASES[k].refused is None])
def test_reference_fp32_meets_the_bar(key):
    """The fp32 numpy oracle's gradient meets the bar against the float64 one, and the float64 batch holds no more ambiguous pairs than
    the cap admits: the inputs and the bar admit a correct fp32 implementation."""
    c = CASES[key]
    train, P, ohp = world(key)
    for short in ((False, True) if c.group == "generic" else (False,)):
        ref = reference(key, short)
        loss32, G32, s32, _ = ko.train_step_grads(c.model, P, ref.batch, dtype=np.float32, **ohp)
        compare(key, ref, G32)
        assert np.isclose(float(loss32), ref.loss, rtol=2e-5), (key, float(loss32), ref.loss)
        assert np.allclose(s32[0], ref.scores[0], atol=2e-5, rtol=2e-5), key


# ------------------------------------------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def hip():
    import torch
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def _trainer(hip, key, monkeypatch, optimizer="sgd", lr=1.0, steps=1, generator=True, tables=world):
    from pykg2vec_amd.trainer import Trainer
    c = CASES[key]
    train, P, _ohp = tables(key)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    cfg = hip.make_config(E, c.R, c.hp, train, train[:8], train[:8], optimizer=optimizer, lr=lr, batch_size=B)
    cfg.tot_train_triples = steps * B
    m = hip.model_from_params(c.model, P, c.hp, E, c.R, train=train)
    tr = Trainer(m, cfg, use_graph=False)
    tr.build_model()
    if generator:
        tr.generator = tr._new_generator()
    return tr, m


def _tables(hip, m):
    return {k[:-len(".weight")]: p.detach().cpu().numpy().copy() for k, p in hip.table_parameters(m)}


def _positives(c, batch):
    if c.pointwise:
        on = np.asarray(batch[3]) > 0
        return tuple(np.asarray(x)[on] for x in batch[:3]), on
    return batch[:3], slice(None)


def _check_forward(hip, c, m, ref, key):
    import torch
    (h, r, t), on = _positives(c, ref.batch)
    with torch.no_grad():
        got = m(hip.dev(h), hip.dev(r), hip.dev(t)).cpu().numpy()
    want = ref.scores[0][on]
    assert np.allclose(got, want, atol=2e-5, rtol=2e-5), (key, float(np.abs(got - want).max()))


def _record(hip, key, worst, ratio, loss, ref):
    hip.record_max("width_edges_deviation", "%s/max_abs" % key, worst)
    hip.record_max("width_edges_deviation", "%s/of_tolerance" % key, ratio)
    hip.record_max("width_edges_deviation", "%s/loss_rel" % key, abs(loss - ref.loss) / abs(ref.loss))


@gpu
@pytest.mark.parametrize("key", STEP_KEYS)
def test_owner_step_at_width_edges_matches_float64(hip, monkeypatch, key):
    """Parts 1 and 1b: one step on the path the case names (or on the path it falls through to), twice."""
    import torch
    from pykg2vec_amd._lib import KgeHipError
    c = CASES[key]
    if c.refused:
        tr, m = _trainer(hip, key, monkeypatch)
        assert tr.step_path(1) == c.path, (key, tr.step_path(1), c.path)
        with pytest.raises((KgeHipError, ValueError), match=c.refused):
            tr.train_model_epoch(0)
        return
    ref = reference(key)
    runs = []
    for i in range(2):
        tr, m = _trainer(hip, key, monkeypatch)
        assert tr.step_path(1) == c.path, (key, tr.step_path(1), c.path)
        if c.group == "pull_two_phase":
            assert tr._pull_two_phase()
        before = _tables(hip, m)
        batch = sb.sampled(tr, B, c.neg, E, c.pointwise)
        assert len(batch) == len(ref.batch) and all(np.array_equal(x, y) for x, y in zip(batch, ref.batch)), key
        if i == 0:
            _check_forward(hip, c, m, ref, key)
        runs.append((tr, before) + sb.one_step(hip, tr, m))
    (tr, before, after, pa, sa, loss), (_tr2, _b2, _a2, pb, sbb, _l2) = runs
    if c.group == "pull_two_phase":
        assert tr._pull.direction is not None
    elif c.path == "pull":
        assert tr._pull.direction is None
    assert np.isclose(loss, ref.loss, rtol=2e-5), (key, loss, ref.loss)
    if c.path != "generic":     # the atomic-free paths reproduce themselves bit for bit
        assert torch.equal(pa, pb) and (sa is None or torch.equal(sa, sbb)), key
    got = {k: before[k].astype(np.float64) - after[k].astype(np.float64) for k in ref.G64}
    worst, ratio = compare(key, ref, got, after)
    _record(hip, key, worst, ratio, loss, ref)


@gpu
@pytest.mark.parametrize("key", GENERIC_KEYS)
def test_generic_step_at_width_edges_matches_float64(hip, monkeypatch, key):
    """The eager, unforced push step on the oracle batch and on its first 37 pairs; gradients read from the flat gradient buffer."""
    import torch
    from pykg2vec_amd._lib import KgeHipError
    c = CASES[key]
    train, P, ohp = world(key)
    for short in (False, True):
        tr, m = _trainer(hip, key, monkeypatch, generator=False)
        assert tr.step_path(1) == "generic", (key, tr.step_path(1))
        step = tr.train_step_pointwise if c.pointwise else tr.train_step_pairwise
        if c.refused:
            batch = oracle_batch(train, 0, c.neg, c.pointwise)
            with pytest.raises((KgeHipError, ValueError), match=c.refused):
                step(*[hip.dev(x) for x in batch])
            return
        ref = reference(key, short)
        if c.model != "rescal":
            _check_forward(hip, c, m, ref, key)
        loss = float(step(*[hip.dev(x) for x in ref.batch]).item())
        torch.cuda.synchronize()
        if c.model == "rescal":     # (its forward renormalises the tables in place: checked on what the step left)
            _check_forward(hip, c, m, ref, key)
        assert np.isclose(loss, ref.loss, rtol=2e-5), (key, short, loss, ref.loss)
        names = [n.split(".")[0] for n, _ in hip.table_parameters(m)]
        got = {n: g.cpu().numpy() for n, g in zip(names, tr.flat.grad_views)}
        worst, ratio = compare(key, ref, got)
        _record(hip, key + ("/ragged" if short else ""), worst, ratio, loss, ref)


@gpu
@pytest.mark.parametrize("key", [k for k, c in CASES.items() if c.group == "own_dword"])
def test_own_dword_form_at_width_edges_matches_float64(hip, monkeypatch, key):
    """Part 1d: DistMult / ComplEx rows of d % 4 != 0 floats through Trainer.own_step_explicit (phase 1 + the in-place SGD step with
    lr = 1 on the touched rows), twice: the same bar, the same loss bound, bit-identical tables."""
    import torch
    from pykg2vec_amd import kernels as K
    c = CASES[key]
    ref = reference(key)
    runs = []
    for i in range(2):
        tr, m = _trainer(hip, key, monkeypatch, generator=False)
        if i == 0:
            _check_forward(hip, c, m, ref, key)
        before = _tables(hip, m)
        tr.loss_buf.zero_()
        tr.own_step_explicit(*[hip.dev(x) for x in ref.batch])
        torch.cuda.synchronize()
        runs.append((before, _tables(hip, m), tr.flat.param.clone(), float(K.read_loss(tr.loss_buf).item())))
    (before, after, pa, loss), (_b, _a, pb, _l) = runs
    assert torch.equal(pa, pb), key
    assert np.isclose(loss, ref.loss, rtol=2e-5), (key, loss, ref.loss)
    got = {k: before[k].astype(np.float64) - after[k].astype(np.float64) for k in ref.G64}
    worst, ratio = compare(key, ref, got, after)
    _record(hip, key, worst, ratio, loss, ref)


@gpu
@pytest.mark.parametrize("model,d", [(m, d) for m in ("hole", "octonione") for d in (252, 256, 257, 260)])
def test_hole_and_octonione_at_width_edges(hip, model, d):
    """HolE (hole_waves) and OctonionE (oct_group) switch at 256: held to their own float64 restatements at the shapes above."""
    if model == "hole":
        from test_hip_kg2e_hole import check_step_vs_float64
        check_step_vs_float64(hip, "hole", E, 5, d, B, seed=d)
    else:
        from test_hip_octonione import bundles, check_step_vs_float64, random_model
        m = random_model(hip, E, 5, d, seed=d)
        check_step_vs_float64(hip, m, E, 5, bundles(np.random.default_rng(d), E, 5, B, 1), B)


# ------------------------------------------------------------------------------------------------------ 1c: optimiser state at the edges
STATE_W = {"pull": (124, 128, 252, 256, 508, 512, 1020, 1024), "own": (124, 128, 252, 256, 508, 512), "ownx": (124, 128, 252, 256),
           "transx": (124, 128, 252, 256, 508, 512), "staged": (252, 256, 1020, 1024, 2044, 2048)}
STATE_KEYS = [k for k, c in CASES.items() if c.group in STATE_W and c.path != "generic" and not c.refused
              and c.hp.get("hidden_size", c.hp.get("ent_hidden_size")) in STATE_W[c.group]
              and not (c.group == "pull" and c.hp["l1_flag"] and c.hp["hidden_size"] > 128)]    # (wide L1: a near-zero residual sign
STATE_LR = 0.01                                                                                   # flips one Adam step outright)


def state_lr(key):
    """Learning rate of a case's three steps.  An excluded element (float64 gradient below NEAR_ZERO) may take the other sign in fp32,
    and Adam's first step then leaves its parameter 2 lr away from the reference's.  In the models whose energy couples the tables
    coordinate by coordinate (the trilinear pointwise models, RotatE) every gradient element of the same coordinate in the rows that
    share a triple with it is proportional to that parameter: with entries of size b it changes by the relative 2 lr / b in the
    following steps, and Adam's update of those -- not excluded -- elements by lr times that.  2 lr^2 / b <= 1e-4 (the bar) needs
    lr <= sqrt(5e-5 b): ~1.5e-3 for RotatE at d = 2048 (b = sqrt(4.5 / d)), ~5e-3 for the pointwise models.  (TransE / TransH /
    TransD rows are normalised before they meet: one coordinate 2 lr off moves every gradient element by 2 lr / ||x|| relative at
    most, ||x|| ~ 1 for these tables: STATE_LR stands.)"""
    c = CASES[key]
    if c.model not in TRILINEAR_TERMS and c.model != "rotate":
        return STATE_LR
    d = c.hp["hidden_size"]
    b = np.sqrt(4.5 / d) if c.model == "rotate" else min(1.0, (27.0 / (TRILINEAR_TERMS[c.model] * d)) ** (1.0 / 6.0))
    return float(min(STATE_LR, np.sqrt(5e-5 * b)))
STATE_EXCLUDED = 2e-3


TRILINEAR_TERMS = {"distmult": 1, "cp": 1, "simple": 1, "simple_ignr": 1, "complex": 4, "analogy": 3, "quate": 16}


def state_world(key):
    """world(key) with the tables of the pointwise models and RotatE rescaled.  At the xavier scale of a 40-entity table the pointwise
    gradients are products of two small entries over the 128 rows of the mean: several per cent of them lie below NEAR_ZERO, where
    Adam's sign-like first step amplifies a rounding residue, and the 0.2 % cap on excluded elements could not hold for any
    implementation.  Entries uniform in +-b with b = min(1, (27 / (T d))^(1/6)) give the sum of T d trilinear terms unit variance (no
    saturated logistic) and gradients of ~b^2 / 128.  RotatE: entity entries in +-sqrt(4.5 / d), so that the squared distance is of
    the size of the margin at every width (its own init, +-(margin + 2) / d, shrinks the gradients like 1 / d)."""
    c = CASES[key]
    train, P, ohp = world(key)
    d = c.hp.get("hidden_size", c.hp.get("ent_hidden_size"))
    P = {k: v.copy() for k, v in P.items()}
    for k, v in P.items():
        if c.model in TRILINEAR_TERMS:
            v *= np.float32(min(1.0, (27.0 / (TRILINEAR_TERMS[c.model] * d)) ** (1.0 / 6.0)) / np.sqrt(6.0 / (v.shape[0] + v.shape[1])))
        elif c.model == "rotate" and k.startswith("ent"):
            v *= np.float32(np.sqrt(4.5 / d) / ((c.hp["margin"] + 2.0) / d))
    return train, P, ohp


@functools.lru_cache(maxsize=16)
def reference_three_steps(key, opt, dtype=np.float64):
    """Three oracle steps (gradient and optimiser in `dtype`) on the epoch's first three batches -> (tables, per-table mask of the
    touched elements, per-table mask of the elements whose gradient was below NEAR_ZERO in some step)."""
    c = CASES[key]
    train, P, ohp = state_world(key)
    P = {k: np.asarray(v, dtype).copy() for k, v in P.items()}
    st = ko.optimizer_init(opt, P)
    touched = {k: np.zeros(v.shape, bool) for k, v in P.items()}
    tiny = {k: np.zeros(v.shape, bool) for k, v in P.items()}
    for s in range(3):
        batch = oracle_batch(train, s, c.neg, c.pointwise)
        _l, G, _s, _ = ko.train_step_grads(c.model, P, batch, dtype=dtype, **ohp)
        G = {k: np.asarray(G.get(k, np.zeros_like(v)), dtype) for k, v in P.items()}
        for k in P:
            touched[k] |= G[k] != 0
            tiny[k] |= (G[k] != 0) & (np.abs(G[k]) < sb.NEAR_ZERO)
        ko.optimizer_step(opt, P, G, st, state_lr(key))
    return P, touched, tiny


def compare_three_steps(key, opt, got):
    """atol = rtol = 1e-4 on every element; an element may miss it only where its float64 gradient was below NEAR_ZERO in one of the
    steps, and such excluded elements are at most STATE_EXCLUDED of the touched ones.  -> (largest deviation kept, excluded)"""
    want, touched, tiny = reference_three_steps(key, opt)
    n_touched = sum(int(t.sum()) for t in touched.values())
    worst, excluded = 0.0, 0
    for k, w in want.items():
        err = np.abs(np.asarray(got[k], np.float64) - w)
        bad = err > 1e-4 + 1e-4 * np.abs(w)
        loud = bad & ~tiny[k]
        assert not loud.any(), (key, opt, k, int(loud.sum()), float(err[loud].max()), np.argwhere(loud)[:4].tolist())
        excluded += int(bad.sum())
        worst = max(worst, float(err[~bad].max()))
    assert excluded <= STATE_EXCLUDED * n_touched, (key, opt, excluded, n_touched)
    return worst, excluded


@pytest.mark.parametrize("opt", ["adam", "adagrad"])
@pytest.mark.parametrize("key", STATE_KEYS)
def test_reference_fp32_three_steps_meet_the_bar(key, opt):
    """The fp32 numpy oracle alone stays inside the three-step bar and the exclusion cap (the seeds are chosen so)."""
    got, _t, _z = reference_three_steps(key, opt, np.float32)
    compare_three_steps(key, opt, got)


@gpu
@pytest.mark.parametrize("opt", ["adam", "adagrad"])
@pytest.mark.parametrize("key", STATE_KEYS)
def test_three_owner_steps_at_width_edges_match_float64(hip, monkeypatch, key, opt):
    import torch
    c = CASES[key]
    tr, m = _trainer(hip, key, monkeypatch, optimizer=opt, lr=state_lr(key), steps=3, tables=state_world)
    assert tr.step_path(3) == c.path, (key, tr.step_path(3), c.path)
    tr.train_model_epoch(0)
    tr.sync_model()
    torch.cuda.synchronize()
    worst, excluded = compare_three_steps(key, opt, _tables(hip, m))
    hip.record_max("width_edges_deviation", "%s/three_steps_%s/max_abs" % (key, opt), worst)
    hip.record_max("width_edges_deviation", "%s/three_steps_%s/excluded" % (key, opt), excluded)


# ------------------------------------------------------------------------------------------------------ 2: optimiser row kernels
OPTS = ["sgd", "adam", "adagrad", "rms"]
OPT_ROWS = [1, 7, 8, 9, 33]      # the 8-row blocks of k_opt_rows4 and the 4-row blocks of k_opt_rows
OPT_D4 = [4, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1020, 1024]
OPT_D1 = [1, 3, 255, 257, 511, 513, 1023]
OPT_LR = 0.01
N_STATES = {"sgd": 0, "adam": 2, "adagrad": 1, "rms": 1}


def opt_inputs(rows, d, seed):
    """Parameters in [-1, 1] and three gradients with |g| in [0.1, 1] and random signs (Adam's and RMSprop's divisions stay well
    conditioned), float32."""
    rng = np.random.default_rng((rows, d, seed))
    n = rows * d
    p = rng.uniform(-1, 1, n).astype(np.float32)
    gs = [(rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(3)]
    return p, gs


def opt_reference(kind, p, gs, dtype, rows=None, d=None, normalize=False):
    """Three ko.optimizer_step steps in `dtype` -> (parameters, states, the parameters as the last update left them).  normalize: every
    row divided by its L2 norm after each update, as k_opt_rows / k_opt_rows4<NORM> document (the row renormalisation Rescal.embed
    would apply at the next forward)."""
    P = {"x": np.asarray(p, dtype).copy()}
    st = ko.optimizer_init(kind, P)
    pre = None
    for g in gs:
        ko.optimizer_step(kind, P, {"x": np.asarray(g, dtype)}, st, OPT_LR)
        pre = P["x"].copy()
        if normalize:
            x = P["x"].reshape(rows, d)
            x /= np.sqrt(np.sum(x * x, axis=1, keepdims=True))
    states = [st[k]["x"] for k in ("m", "v", "sq") if k in st]
    return P["x"], states, pre


@pytest.mark.parametrize("kind", OPTS)
def test_reference_optimizer_fp32_meets_the_flat_bound(kind):
    """ko.optimizer_step in fp32 stays within atol = rtol = 1e-6 of its own float64 run on these inputs: the bound the flat device
    form is held to admits a correct fp32 implementation."""
    for d in (4, 257, 1024):
        p, gs = opt_inputs(9, d, 0)
        p32, s32, _ = opt_reference(kind, p, gs, np.float32)
        p64, s64, _ = opt_reference(kind, p, gs, np.float64)
        assert np.allclose(p32, p64, atol=1e-6, rtol=1e-6), (kind, d, float(np.abs(p32 - p64).max()))
        for a, b in zip(s32, s64):
            assert np.allclose(a, b, atol=1e-6, rtol=1e-6), (kind, d)


def _dev_buffers(kind, p, offset):
    """param, grad, state1, state2 on the device; offset: every buffer is a view one float into its allocation (4-byte aligned only)."""
    import torch

    def buf(init=None):
        base = torch.zeros(len(p) + 4, dtype=torch.float32, device="cuda")
        v = base[1:1 + len(p)] if offset else base[:len(p)]
        assert v.data_ptr() % 16 == (4 if offset else 0)
        if init is not None:
            v.copy_(torch.from_numpy(init))
        return v
    ns = N_STATES[kind]
    return buf(p), buf(), (buf() if ns >= 1 else None), (buf() if ns >= 2 else None)


def _three_device_steps(K, kind, p, gs, rows=None, d=None, offset=False, normalize=False, touched=None, clear=None):
    """Three steps of the flat form (rows is None) or the row form; the gradient buffer must come back zeroed where it was read."""
    import torch
    param, grad, s1, s2 = _dev_buffers(kind, p, offset)
    for step, g in enumerate(gs, 1):
        grad.copy_(torch.from_numpy(g))
        if rows is None:
            K.optimizer_step(kind, param, grad, s1, s2, OPT_LR, step, zero_grad=True)
        else:
            K.optimizer_step_rows(kind, param, grad, s1, s2, rows, d, OPT_LR, step, zero_grad=True, normalize=normalize,
                                  touched=touched, touched_clear=clear)
        assert not bool(grad.any()), (kind, rows, d, "gradient not zeroed")
    torch.cuda.synchronize()
    return param, s1, s2


@gpu
@pytest.mark.parametrize("d", OPT_D4 + OPT_D1)
@pytest.mark.parametrize("kind", OPTS)
def test_optimizer_rows_equal_the_flat_form_bit_for_bit(hip, kind, d):
    """k_opt_rows4<NV> (d % 4 == 0) / k_opt_rows<NCH> (any other d) against k_opt on identical buffers: both apply opt_update<KIND> per
    element with no reduction, so parameter, both states and the zeroed gradient are identical after three steps.  The flat form
    itself is held to ko.optimizer_step in float64 at atol = rtol = 1e-6."""
    import torch
    from pykg2vec_amd import kernels as K
    for rows in OPT_ROWS:
        p, gs = opt_inputs(rows, d, 1)
        flat = _three_device_steps(K, kind, p, gs)
        by_rows = _three_device_steps(K, kind, p, gs, rows, d)
        for what, a, b in zip(("param", "state1", "state2"), flat, by_rows):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (kind, rows, d, what)
        p64, s64, _ = opt_reference(kind, p, gs, np.float64)
        got = flat[0].cpu().numpy()
        assert np.allclose(got, p64, atol=1e-6, rtol=1e-6), (kind, rows, d, float(np.abs(got - p64).max()))
        for a, b in zip([x for x in flat[1:] if x is not None], s64):
            assert np.allclose(a.cpu().numpy(), b, atol=1e-6, rtol=1e-6), (kind, rows, d, "state")
        hip.record_max("width_edges_deviation", "opt_flat/%s/d%d/max_abs" % (kind, d), float(np.abs(got - p64).max()))


@gpu
@pytest.mark.parametrize("d", [128, 512, 1024])
@pytest.mark.parametrize("kind", OPTS)
def test_optimizer_rows_on_four_byte_aligned_views_take_the_dword_form(hip, kind, d):
    """Buffers one float into their allocations (d % 4 == 0): rows4_ok refuses them (csrc/kge_opt.hip:324-326), the dword kernel
    serves, and the result is still the flat form's bit for bit."""
    import torch
    from pykg2vec_amd import kernels as K
    for rows in (9, 33):
        p, gs = opt_inputs(rows, d, 2)
        flat = _three_device_steps(K, kind, p, gs)
        by_rows = _three_device_steps(K, kind, p, gs, rows, d, offset=True)
        for what, a, b in zip(("param", "state1", "state2"), flat, by_rows):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (kind, rows, d, what)


@gpu
def test_optimizer_rows_refuse_rows_of_1025_floats(hip):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd._lib import KgeHipError
    p, gs = opt_inputs(3, 1025, 3)
    with pytest.raises(KgeHipError, match="rows of at most 1024 floats"):
        _three_device_steps(K, "adam", p, gs, 3, 1025)


@gpu
@pytest.mark.parametrize("d", OPT_D4 + OPT_D1)
@pytest.mark.parametrize("kind", OPTS)
def test_optimizer_rows_renormalise_like_float64(hip, kind, d):
    """normalize=True: update, then store the row divided by its L2 norm, against the float64 restatement of the same.

    Bound per element of a row x (after the update) with norm n and normalised value x^ = x / n:
      the fp32 update is within dx_i = 1e-6 (1 + |x_i|) of float64 (the flat bound above), which moves x^_i by at most
      dx_i / n + |x^_i| ||dx||_2 / n (the row's own error and the norm's);
      the fp32 norm: a sum of d squares in any order is within (d - 1) 2^-24 relative of the exact one (each square one more rounding:
      d 2^-24), the square root halves that and rounds once, the division rounds once: at most (d + 2) 2^-24 relative, plus the one
      rounding of the stored quotient.
    So |got - want| <= (dx_i + |x^_i| ||dx||_2) / n + |x^_i| (d + 3) 2^-24.  Each later step starts from the stored fp32 row, whose
    deviation is of the same size and enters dx: three steps, three times the bound."""
    from pykg2vec_amd import kernels as K
    for rows in OPT_ROWS:
        p, gs = opt_inputs(rows, d, 4)
        got = _three_device_steps(K, kind, p, gs, rows, d, normalize=True)[0].cpu().numpy().reshape(rows, d)
        want, _s, pre = opt_reference(kind, p, gs, np.float64, rows, d, normalize=True)
        want, x = want.reshape(rows, d), pre.reshape(rows, d)
        n = np.sqrt(np.sum(x * x, axis=1, keepdims=True))
        dx = 1e-6 * (1 + np.abs(x))
        tol = 3 * ((dx + np.abs(want) * np.sqrt(np.sum(dx * dx, axis=1, keepdims=True))) / n + np.abs(want) * (d + 3) * 2.0 ** -24)
        err = np.abs(got - want)
        assert (err <= tol).all(), (kind, rows, d, float((err / tol).max()), float(err.max()))
        hip.record_max("width_edges_deviation", "opt_rows_norm/%s/d%d/of_tolerance" % (kind, d), float((err / tol).max()))


@gpu
@pytest.mark.parametrize("d", OPT_D4 + OPT_D1)
@pytest.mark.parametrize("kind", OPTS)
def test_optimizer_rows_leave_untouched_rows_alone(hip, kind, d):
    """Touched-bitmap form: rows whose bit is clear (their gradient rows are zero: the bitmap lists the rows with a gradient) are
    bit-unchanged in the parameter and in both states; the rows whose bit is set equal the flat form's; the other parity's bitmap
    comes back cleared."""
    import torch
    from pykg2vec_amd import kernels as K
    rows = 33
    p, gs = opt_inputs(rows, d, 5)
    on = np.random.default_rng(d).random(rows) < 0.5
    on[[0, 32]] = [True, False]
    gs = [(g.reshape(rows, d) * on[:, None]).reshape(-1).astype(np.float32) for g in gs]
    words = np.zeros(2, np.uint32)
    for r in np.flatnonzero(on):
        words[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    touched = torch.from_numpy(words.view(np.int32).copy()).cuda()
    clear = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    flat = _three_device_steps(K, kind, p, gs)
    by_rows = _three_device_steps(K, kind, p, gs, rows, d, touched=touched, clear=clear)
    assert not bool(clear.any()), (kind, d, "the other parity's bitmap is not cleared")
    off = torch.from_numpy(~on).cuda()
    start = torch.from_numpy(p).cuda().view(rows, d)
    for what, a, b in zip(("param", "state1", "state2"), flat, by_rows):
        if a is None:
            continue
        assert torch.equal(a, b), (kind, d, what)
        before = start if what == "param" else torch.zeros_like(start)
        assert torch.equal(b.view(rows, d)[off], before[off]), (kind, d, what, "an untouched row moved")


if __name__ == "__main__":      # the seed search behind SEEDS: float64 oracle only
    found = {}
    for key_, c_ in CASES.items():
        if c_.refused or c_.model not in sb.HINGE:
            continue
        train_ = train_split(c_.R)
        batch_ = oracle_batch(train_, 0, c_.neg, c_.pointwise)
        for seed_ in range(2000):
            _t, P_, ohp_ = world(key_, seed_)
            if quick_ambiguous(c_, P_, batch_, ohp_) == 0:
                break
        else:
            raise SystemExit("no seed for %s" % key_)
        if seed_:
            found[key_] = seed_
    print("SEEDS = %r" % found)
