"""Batch compositions, dispatch plan, grouping reference and case lists for tests/test_hip_relgroup_edges.py (numpy only, no GPU).

RESCAL and TransR train through a device-side grouping of the batch by relation (csrc/kge_relgroup.h; group_by_relation_split and its
kernels at the top of csrc/kge_dense.hip).  Every step form behind it indexes its work by offsets / tile_off / tile_rel / perm, and
what happens to a batch is decided by integer thresholds on the number of pairs n, the relation count R and the per-relation count
n_r.  This file states

    composition()    a pair batch (ph, pr, pt, nh, pr, nt) whose relation i holds exactly counts[i] pairs, in one of three orders;
    plan()           which grouping form and which step form the library takes for (model, n, R, k, switches): a restatement of the
                     host code, every rule cited by source line.  It is used only to name the kernels a case is meant to reach and to
                     assert that the case lists leave no reachable (grouping form, step form) cell empty; never an oracle for values;
    grouping_ref()   the numpy answer for the four arrays.  No entry point of the library hands them out (the grouping lives in the
                     steps' workspaces), so on the GPU the step results carry the check; here it pins what composition() promises;
    the case lists   A (per-relation counts at the tile edges), B (the sorted grouping), C (the scans), D (the step-form thresholds),
                     G (every step form behind the block-aggregated and the global-atomic grouping), E (grouped ranks).

The float64 side of a case (reference()) is kge_oracle.train_step_grads under the per-row bar of tests/step_bar.py, taken unchanged.
The hinge allowance of that bar is a condition here, not a measurement: the tables of every case come from the first table seed
(0, 1, 2, ...: table_seed(), searched on the float64 oracle alone) for which no pair lies within NEAR_MARGIN of the margin and, for
L1 TransR, no residual component of any pair lies within NEAR_ZERO of zero.  reference() asserts that the allowance is then exactly
zero: no element of any case is excused."""
import collections
import functools
import zlib

import numpy as np

import kge_oracle as ko
import step_bar as sb

# ---- constants of the device code, copied from the sources (never from a kernel's results)
TILE = 32                   # csrc/kge_relgroup.h:9        triples per tile of k_rescal<MODE> / the TransR tile kernels
PAIR_TILE = 16              # csrc/kge_relgroup.h:10       kPairTile: k_rescal_pair, k_rescal_rows, k_rescal_g / g2 / pair_gm
SLAB_CHUNK = 64             # csrc/kge_relgroup.h:11       kSlabChunk: pairs per chunk of the slab form
TR_PAIR_TILE = 16           # csrc/kge_transr_rows.hip:30  kTrPairTile (a workgroup of k_transr_rows takes two)
TR_G_RUN = 8                # csrc/kge_transr_rows.hip:31  kTrGRun: tiles per run of k_transr_g (shared_rel from n_r > 128, :442)
G_RUN = 8                   # csrc/kge_dense.hip:1167      kGRun: tiles per run of k_rescal_g / g2 (shared_rel from n_r > 128, :1185)
GROUP_ITEMS = 4096          # csrc/kge_dense.hip:69        kGroupItems: items per block of k_rel_hist_lds / k_rel_scatter_lds
SMALL_MAX_R = 4096          # csrc/kge_dense.hip:116       kSmallGroupMaxR
SMALL_MAX_N = 16384         # csrc/kge_dense.hip:117       kSmallGroupMaxN
STAGE_MAX_N = 4096          # csrc/kge_dense.hip:118       kStageMaxN
SMALL_SCAN = 1024           # csrc/kge_dense.hip:156       relations per scan pass of k_rel_group_small (carry in s_carry)
SCAN = 256                  # csrc/kge_dense.hip:36        relations per pass of k_rel_scan
SORT_MIN, SORT_MAX = 2, 64  # csrc/kge_dense.hip:196       relations the bitonic network sorts
SPLIT_N, SPLIT_MANY_N, MANY_R = 8192, 512, 512      # csrc/kge_dense.hip:1455  kPairSplitG, kPairSplitManyRel, kManyRelations
STAGE_LDS = 64 * 1024 - 64  # csrc/kge_dense.hip:1496      (3 R + 2 n + 2) * 4 <= this

SWITCHES = ("KGE_RESCAL_FUSED", "KGE_RESCAL_UNFUSED", "KGE_RESCAL_STAGED", "KGE_RESCAL_SLAB", "KGE_RESCAL_SPLIT_MIN", "KGE_RESCAL_ROWS",
            "KGE_RESCAL_G", "KGE_RESCAL_G2", "KGE_TRANSR_ROWS", "KGE_TRANSR_G")


# --------------------------------------------------------------------------------------------------------------- compositions
Batch = collections.namedtuple("Batch", "ph pr pt nh nr nt E R counts order")
ORDERS = ("sorted", "shuffled", "interleaved")


def entity_count(n):
    """Entities of a composition of n pairs: 4 n incidences over n / 3 rows, so rows repeat across tiles at every size."""
    return max(16, n // 3)


def composition(counts, seed, order):
    """A pair batch whose relation i holds exactly counts[i] pairs (zeros anywhere).  The pairs are drawn in relation order first --
    positives pairwise distinct; every fifth pair repeats its neighbour's head and every seventh its neighbour's tail, so rows repeat
    inside a tile; a negative replaces the head or the tail by another entity -- and then laid out "sorted", "shuffled" (relations
    interleaved at random), or "interleaved" (round robin over the relations: every 4096-item block of the block-aggregated grouping
    sees every relation that still has pairs).  The same (counts, seed) gives the same set of pairs in every order."""
    assert order in ORDERS, order
    counts = np.asarray(counts, dtype=np.int64)
    R, n = len(counts), int(counts.sum())
    assert R >= 1 and n >= 1 and (counts >= 0).all()
    E = entity_count(n)
    rng = np.random.default_rng([int(seed), n, R])
    pr = np.repeat(np.arange(R, dtype=np.int64), counts)
    ph, pt = rng.integers(E, size=n), rng.integers(E, size=n)
    g = np.arange(n)
    same = np.concatenate([[False], pr[1:] == pr[:-1]])
    for col, m, off in ((ph, 5, 1), (pt, 7, 3)):
        at = np.flatnonzero(same & (g % m == off))
        col[at] = col[at - 1]
    for _ in range(64):            # positives pairwise distinct (the train split is a set)
        code = (pr * E + ph) * E + pt
        _u, first = np.unique(code, return_index=True)
        dup = np.setdiff1d(g, first)
        if not len(dup):
            break
        pt[dup] = rng.integers(E, size=len(dup))
    else:
        raise AssertionError("composition: duplicate positives remain")
    tail = rng.random(n) < 0.5
    other = rng.integers(E - 1, size=n)
    nh = np.where(tail, ph, (ph + 1 + other) % E)
    nt = np.where(tail, (pt + 1 + other) % E, pt)
    if order == "shuffled":
        # the relations' pairs interleaved at random, each relation's own pairs in drawing order: a grouping that sorts a relation by
        # pair index then arrives at the grouped order of "sorted" (what case set B holds the staged step to, bit for bit)
        lab = pr[np.random.default_rng([int(seed), n, R, 1]).permutation(n)]
        idx = np.empty(n, dtype=np.int64)
        idx[np.argsort(lab, kind="stable")] = g
    elif order == "interleaved":
        within = g - np.repeat(np.cumsum(counts) - counts, counts)
        idx = np.lexsort((pr, within))
    else:
        idx = g
    out = [np.ascontiguousarray(x[idx], dtype=np.int64) for x in (ph, pr, pt, nh, pr, nt)]
    return Batch(*out, E, R, tuple(int(c) for c in counts), order)


def grouping_ref(r, R, tile):
    """(offsets [R + 1], tile_off [R + 1], members: per relation the ascending array of the rows perm holds inside its range -- the
    multiset; the order inside a range is arrival order but for the sorted form --, tile_rel [tile_off[R]])."""
    r = np.asarray(r, dtype=np.int64)
    counts = np.bincount(r, minlength=R)
    tiles = -(-counts // tile)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    tile_off = np.concatenate([[0], np.cumsum(tiles)])
    members = [np.flatnonzero(r == rel) for rel in range(R)]
    tile_rel = np.repeat(np.arange(R), tiles)
    assert tile_off[R] <= len(r) // tile + R + 1          # group_max_tiles (csrc/kge_relgroup.h:22)
    return offsets, tile_off, members, tile_rel


MISTAKES = ("drop_last", "lost_carry", "tile_rel_at_1", "padding_zero", "full_tile")


def consumed_pairs(r, R, tile, mistake=None, scan=SMALL_SCAN, sort=False):
    """A value-level model of the grouping and of how a step walks it, with one deliberate mistake: [(relation used, pair)] in the order
    the tiles consume them.  drop_last: offsets[rel + 1] - 1 ends the heaviest relation; lost_carry: every scan pass starts from 0;
    tile_rel_at_1: tile_rel is written by the pair with local % tile == 1 (other tiles keep the 0 the buffer held); padding_zero: the
    bitonic network pads with 0 (sort: relations of 2 .. 64 pairs are sorted by pair index); full_tile: every tile claims `tile` pairs.
    Positions outside [0, n) and positions nothing wrote are skipped here (the device would read whatever lies there)."""
    r = np.asarray(r, dtype=np.int64)
    n = len(r)
    counts = np.bincount(r, minlength=R)
    tiles = -(-counts // tile)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    tile_off = np.concatenate([[0], np.cumsum(tiles)])
    if mistake == "lost_carry":
        for base in range(scan, R, scan):
            offsets[base:base + scan] -= offsets[base]
            tile_off[base:base + scan] -= tile_off[base]
    perm = np.full(n, -1, dtype=np.int64)
    tile_rel = np.zeros(n // tile + R + 1, dtype=np.int64)
    cursor = np.zeros(R, dtype=np.int64)
    for i in range(n):
        rel = r[i]
        local = cursor[rel]
        cursor[rel] += 1
        perm[offsets[rel] + local] = i
        if local % tile == (1 if mistake == "tile_rel_at_1" else 0):
            tile_rel[tile_off[rel] + local // tile] = rel
    if sort:
        for rel in range(R):
            lo, c = offsets[rel], counts[rel]
            if SORT_MIN <= c <= SORT_MAX:
                pad = 0 if mistake == "padding_zero" else 0x7FFFFFFF
                perm[lo:lo + c] = np.sort(np.concatenate([perm[lo:lo + c], np.full(64 - c, pad)]))[:c]
    heavy = int(np.argmax(counts))
    out = []
    for b in range(int(np.sum(tiles))):
        rel = int(tile_rel[b])
        tin = b - tile_off[rel]
        end = offsets[rel + 1] - (1 if mistake == "drop_last" and rel == heavy else 0)
        g0 = offsets[rel] + tin * tile
        cnt = tile if mistake == "full_tile" else min(tile, end - g0)
        if tin < 0:
            continue
        out += [(rel, int(perm[g])) for g in range(g0, g0 + cnt) if 0 <= g < n and perm[g] >= 0]
    return out


def group_max_tiles_ok(counts, tile):
    """The tiles of a composition fit group_max_tiles (csrc/kge_relgroup.h:22: n / TILE + R + 1)."""
    counts = np.asarray(counts)
    return int((-(-counts // tile)).sum()) <= int(counts.sum()) // tile + len(counts) + 1


# --------------------------------------------------------------------------------------------------------------- the plan
def _sw(env, name):
    """switch_value (csrc/kge_debug.hip:20-28): -1 when unset or empty, else atoi."""
    v = (env or {}).get("KGE_" + name, "")
    return int(v) if v != "" else -1


def _flag(env, name):
    """Trainer._switches (pykg2vec_amd/trainer.py:58): None when unset, else == "1"."""
    v = (env or {}).get(name)
    return None if v is None else v == "1"


def grouping_form(n, R, zero_n=0, sorted_=False):
    """group_by_relation_split (csrc/kge_dense.hip:249-278) for n items."""
    if n <= SMALL_MAX_N and R <= SMALL_MAX_R and zero_n <= SMALL_MAX_N:                 # :251
        return "small_sorted" if sorted_ else "small"                                   # k_rel_group_small (:119-245)
    if R <= SMALL_MAX_R:                                                                # :265
        return "lds"                                                                    # k_rel_hist_lds / k_rel_scan / k_rel_scatter_lds
    return "atomic"                                                                     # :273-277 k_rel_hist / k_rel_scan / k_rel_scatter


def pair_split(n, R, env):
    """pair_split (csrc/kge_dense.hip:1456-1460)."""
    v = _sw(env, "RESCAL_SPLIT_MIN")
    if v > 0:
        return n >= v
    return n >= SPLIT_N or (R >= MANY_R and n >= SPLIT_MANY_N)


def rescal_slab_taken(n, R, k, env):
    """rescal_slab_taken (csrc/kge_dense.hip:1487-1492) with rescal_slab_extra_bytes (:1476-1480); the workspace is the one
    kge_workspace_bytes sizes (csrc/kge_api.hip:146-154), which holds the slab's share whenever that is non-zero."""
    extra = k % 2 == 0 and k <= 256 and n < SPLIT_N and grouping_form(n, R) == "small"
    return (not pair_split(n, R, env)) and extra and _sw(env, "RESCAL_SLAB") != 0


def rescal_stage_ok(n, R, k, env):
    """rescal_stage_ok (csrc/kge_dense.hip:1493-1498)."""
    return k % 4 == 0 and n <= STAGE_MAX_N and (3 * R + 2 * n + 2) * 4 <= STAGE_LDS and rescal_slab_taken(n, R, k, env)


Plan = collections.namedtuple("Plan", "grouping items tile step kernels staged scan_passes")


def _scan_passes(form, R):
    return -(-R // (SMALL_SCAN if form.startswith("small") else SCAN))


def _plan(form_args, tile, step, kernels, staged=False):
    n_items, R, zero_n, sorted_ = form_args
    form = grouping_form(n_items, R, zero_n, sorted_)
    return Plan(form, n_items, tile, step, tuple(kernels), staged, _scan_passes(form, R))


def plan(model, n, R, k, env=None):
    """What one Trainer step of n pairs (neg_rate 1: the negatives share the positives' relation buffer, trainer.py:188-191) runs.
    k: RESCAL's hidden size, or (d_e, d_r) for TransR.  Entity tables are far below 32 MB here, so Trainer._rescal_fused is what
    KGE_RESCAL_FUSED says (trainer.py:759-769); table pointers are 16-byte aligned (torch allocations)."""
    env = env or {}
    if model == "transr":
        de, dr = k
        rows_sw = _sw(env, "TRANSR_ROWS")
        # transr_pair_fast (csrc/kge_transr_rows.hip:801-808; kTransRRowsMinPairs = 1, :798); transr_rows_ok (:716-730: widths <= 128)
        if rows_sw != 0 and n >= 1 and de <= 128 and dr <= 128:
            vec = (de | dr) % 4 == 0                                                     # :734-735
            g = "k_transr_g2" if vec and _sw(env, "TRANSR_G") != 0 else "k_transr_g"     # :753-758
            return _plan((n, R, 0, False), TR_PAIR_TILE, "rows+" + g[len("k_transr_"):], ("k_transr_rows", g))      # :768
        # the tile kernels over the 2 n triples of both sides (csrc/kge_api.hip:219-224, csrc/kge_transr.hip:282-292)
        return _plan((2 * n, R, 0, False), TILE, "tiles32", ("k_transr<0>", "k_hinge_coeffs", "k_transr<1>"))
    assert model == "rescal", model
    fused = _flag(env, "KGE_RESCAL_FUSED") is True                                      # trainer.py:765-769
    unfused = _flag(env, "KGE_RESCAL_UNFUSED") is True                                  # trainer.py:193, csrc/kge_dense.hip:1580
    pair_ok = k % 2 == 0 and k <= 256                                                   # rescal_pair_step_ok (:1482-1484)
    if not pair_ok or unfused:
        # kge_train_pairwise_hinge: forward over 2 n triples (clears the 2 n scores on the way, :484), coefficients, backward
        # (csrc/kge_api.hip:219-224, csrc/kge_dense.hip:471-509)
        return _plan((2 * n, R, 2 * n, False), TILE, "tiles32", ("k_rescal<0>", "k_hinge_coeffs", "k_rescal_gm", "k_rescal<1>"))
    # launch_rescal_pair_step (csrc/kge_dense.hip:1500-1573), entered from the Trainer (trainer.py:193-205) or rescal_pair_fast (:1577-1584)
    stage = fused and _flag(env, "KGE_RESCAL_STAGED") is not False and rescal_stage_ok(n, R, k, env)    # trainer.py:771-784
    if rescal_slab_taken(n, R, k, env):                                                 # :1512-1521
        return _plan((n, R, 0, stage), SLAB_CHUNK, "slab_staged" if stage else "slab", ("rescal_slab",), staged=stage)
    split = pair_split(n, R, env)                                                       # :1534
    rows = split and k <= 208 and _sw(env, "RESCAL_ROWS") != 0                          # :1538
    g_sw = _sw(env, "RESCAL_G")
    g2_ok = k % 4 == 0 and _sw(env, "RESCAL_G2") != 0                                   # :1554
    gemm_g = rows and (g_sw == 1 if g_sw >= 0 else (g2_ok or n >= 128 * R))             # :1555
    pair = "k_rescal_pair<%d>" % (4 if k % 4 == 0 else 2)                               # :1565
    kernels = ["k_rescal_rows" if rows else pair]                                       # :1539-1549, :1558-1560
    step = "rows" if rows else "pair"
    if split and not gemm_g:                                                            # :1561-1563
        kernels.append("k_rescal_pair_gm")
        step += "+gm"
    if gemm_g:                                                                          # :1567-1571, launch_rescal_g (:1436-1449)
        ja = ((k + 15) // 16 + 1) // 2
        vec = k % 4 == 0 and k >= 16 * ja + 4                                           # :1440: the 16-byte gather needs k >= 20
        g = "k_rescal_g2" if vec and _sw(env, "RESCAL_G2") != 0 else "k_rescal_g"
        kernels.append(g)
        step += "+" + g[len("k_rescal_"):]
    return _plan((n, R, 0, False), PAIR_TILE, step, kernels)


# --------------------------------------------------------------------------------------------------------------- switch sets
BIG = str(1 << 30)
RESCAL_ENVS = collections.OrderedDict([
    ("default", {}),
    ("slab0", {"KGE_RESCAL_SLAB": "0"}),
    ("nosplit", {"KGE_RESCAL_SLAB": "0", "KGE_RESCAL_SPLIT_MIN": BIG}),     # k_rescal_pair alone where the default rule splits
    ("split", {"KGE_RESCAL_SPLIT_MIN": "1"}),
    ("split_g0", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_G": "0"}),
    ("split_g1", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_G": "1"}),
    ("split_g2_0", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_G2": "0"}),
    ("split_g1_g2_0", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_G": "1", "KGE_RESCAL_G2": "0"}),
    ("split_g2_1", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_G2": "1"}),
    ("split_rows0", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_ROWS": "0"}),
    ("split_rows0_g1", {"KGE_RESCAL_SPLIT_MIN": "1", "KGE_RESCAL_ROWS": "0", "KGE_RESCAL_G": "1"}),
    ("unfused", {"KGE_RESCAL_UNFUSED": "1"}),
    ("staged", {"KGE_RESCAL_FUSED": "1", "KGE_RESCAL_STAGED": "1"}),
    # (R >= 512 splits from 512 pairs on and R < 512 leaves 3 R + 2 n + 2 far below the LDS bound at n <= 4096: the bound binds only
    # where the split rule is switched off)
    ("staged_nosplit", {"KGE_RESCAL_FUSED": "1", "KGE_RESCAL_STAGED": "1", "KGE_RESCAL_SPLIT_MIN": BIG}),
])
TRANSR_ENVS = collections.OrderedDict([
    ("default", {}), ("rows0", {"KGE_TRANSR_ROWS": "0"}), ("rows1", {"KGE_TRANSR_ROWS": "1"}), ("rows2", {"KGE_TRANSR_ROWS": "2"}),
    ("g0", {"KGE_TRANSR_G": "0"}),
])
ENVS = {"rescal": RESCAL_ENVS, "transr": TRANSR_ENVS}
TRANSR_DIMS = ((8, 12, True), (12, 8, False))      # (d_e, d_r, L1): both row-kernel instantiations of the norm


# --------------------------------------------------------------------------------------------------------------- the cases
TILE_EDGE_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
A_COUNTS = collections.OrderedDict([
    ("edges", TILE_EDGE_COUNTS),
    ("edges_rev", TILE_EDGE_COUNTS[::-1]),                                    # the empty relation last
    ("edges_gap", TILE_EDGE_COUNTS[1:8] + (0, 0) + TILE_EDGE_COUNTS[8:]),     # two empty relations in a row in the middle
] + [("one_rel_%d" % n, (n,)) for n in (1, 16, 17, 64, 65, 129)] + [
    ("ones_300", (1,) * 300),                                                 # tiles = n: the n / tile + R + 1 bound nearly met
    ("last_300", (0,) * 299 + (300,)),
])
B_COUNTS = collections.OrderedDict([
    ("sortable", (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 0, 2, 64, 1)),     # A's counts up to 64, with 1, 2, 63 and 64
    ("one_65", (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 0, 2, 65, 1)),       # one relation beyond the network
])
SCAN_R = (255, 256, 257, 1023, 1024, 1025, 2049, 4095, 4096, 4097)
SCAN_CYCLE = (2, 17, 0, 1)       # the cycle (0, 1, 2, 17), started so that the empty relation is 4 j + 2
SCAN_CYCLE_SPARSE = SCAN_CYCLE + (2, 3, 0, 1) * 3      # R > 2048: the 17 in every sixteenth relation, so that n stays below 16384


def scan_counts(R, n_min=None):
    """Counts cycling through (0, 1, 2, 17), started at 2: every pass boundary of both scans is a multiple of 4, so the relation before
    it (4 j - 1) holds 1 pair and the one after it (4 j) holds 2 -- both non-empty -- and both carried sums (pairs, and tiles of 16,
    32 or 64) are non-trivial at every boundary.  The cycle's own mean is 5, so n = 5 R (3 R / 2 cannot hold a 17 in every four
    relations); above R = 2048 three cycles in four carry a 3 in place of the 17 (n = 2.4 R), which keeps R = 4095 and 4096 inside
    the one-launch grouping (n <= 16384), where its scan takes four passes.
    n_min: the non-empty relations are raised evenly until the sum reaches it (n just above 16384)."""
    cyc = np.asarray(SCAN_CYCLE if R <= 2048 else SCAN_CYCLE_SPARSE, dtype=np.int64)
    c = cyc[np.arange(R) % len(cyc)].copy()
    if n_min is not None and c.sum() < n_min:
        live = np.flatnonzero(c > 0)
        add = n_min - int(c.sum())
        c[live] += add // len(live)
        c[live[:add % len(live)]] += 1
    return tuple(int(x) for x in c)


def _even_counts(n, R):
    """n pairs over R relations as evenly as they go (the first n % R relations hold one more)."""
    return tuple(n // R + (1 if i < n % R else 0) for i in range(R))


Case = collections.namedtuple("Case", "key cls model dims l1 counts order envname env seed")
CASES = collections.OrderedDict()


def _dims_key(model, dims):
    return "k%d" % dims if model == "rescal" else "d%dx%d" % dims


def add_case(cls, name, model, dims, l1, counts, order, envname, seed=0):
    key = "%s/%s/%s/%s/%s/%s" % (cls, model, name, _dims_key(model, dims), order, envname)
    assert key not in CASES, key
    CASES[key] = Case(key, cls, model, dims, l1, tuple(counts), order, envname, ENVS[model][envname], seed)
    return key


def case_plan(c):
    return plan(c.model, sum(c.counts), len(c.counts), c.dims, c.env)


def distinct_envs(model, n, R, dims, names=None):
    """The switch sets that lead (n, R) to pairwise different launches, in ENVS order (the first of equals is kept)."""
    seen, out = set(), []
    for name, env in ENVS[model].items():
        if names is not None and name not in names:
            continue
        p = plan(model, n, R, dims, env)
        sig = (p.grouping, p.tile, p.step, p.kernels, p.staged)
        if sig not in seen:
            seen.add(sig)
            out.append(name)
    return out


def _add_all_forms(cls, name, counts, order, i, extra_k=()):
    """One composition through every step form its (n, R) can reach by the switches; hidden sizes alternate with i."""
    n, R = sum(counts), len(counts)
    for k in (8, 12)[i % 2:i % 2 + 1] + tuple(extra_k):
        names = None
        if k == 6:      # float2 rows: k_rescal_pair<2> and the dword k_rescal_g (and what else differs at k % 4 != 0)
            names = ("slab0", "nosplit", "split", "split_g1", "split_rows0", "split_rows0_g1", "default")
        if k == 20:     # the 16-byte gather k_rescal_g2 needs k >= 20 (launch_rescal_g)
            names = ("split", "split_g2_0", "split_g1_g2_0")
        for envname in distinct_envs("rescal", n, R, k, names):
            add_case(cls, name, "rescal", k, False, counts, order, envname)
    de, dr, l1 = TRANSR_DIMS[i % 2]
    for envname in TRANSR_ENVS:        # (KGE_TRANSR_ROWS = 1 and 2 launch what the default does: the issue lists them, they run)
        add_case(cls, name, "transr", (de, dr), l1, counts, order, envname)


# A: per-relation counts at the tile edges, every step form
for _i, (_name, _counts) in enumerate(A_COUNTS.items()):
    _add_all_forms("A", _name, _counts, "shuffled", _i, extra_k=(6, 20) if _name == "edges" else ())

# B: the sorted grouping (the GPU test adds the bit-for-bit runs); n = 4096 / 4097; the LDS bound 3 R + 2 n + 2 <= 16368 on both sides
for _name, _counts in B_COUNTS.items():
    for _order in ("shuffled", "sorted"):
        add_case("B", _name, "rescal", 8, False, _counts, _order, "staged")
add_case("B", "n4096", "rescal", 8, False, _even_counts(4096, 40), "shuffled", "staged")
add_case("B", "n4097", "rescal", 8, False, _even_counts(4097, 40), "shuffled", "staged")
_R_LDS = (STAGE_LDS // 4 - 2 - 2 * 3600) // 3
B_LDS = ((3600, _R_LDS), (3600, _R_LDS + 1))          # (n, R): the last shape inside the bound and the first beyond it
for _n, _R in B_LDS:
    add_case("B", "lds_n%d_R%d" % (_n, _R), "rescal", 12, False, _even_counts(_n, _R), "shuffled", "staged_nosplit")

# C: the scans -- the second, third ... pass of both scan kernels, and the global-atomic grouping at R = 4097
for _i, _R in enumerate(SCAN_R):
    add_case("C", "scan_R%d" % _R, "rescal", (8, 12)[_i % 2], False, scan_counts(_R), "shuffled", "default")
    _de, _dr, _l1 = TRANSR_DIMS[_i % 2]
    add_case("C", "scan_R%d" % _R, "transr", (_de, _dr), _l1, scan_counts(_R), "shuffled", "default")
    add_case("C", "scan_big_R%d" % _R, "rescal", 8, False, scan_counts(_R, 16385 + _i), "interleaved", "default")
    add_case("C", "scan_big_R%d" % _R, "transr", (8, 8), False, scan_counts(_R, 16385 + _i), "interleaved", "default")

# D: both sides of every step-form threshold
D_SHAPES = collections.OrderedDict([
    ("n8191_R40", (8191, 40, {})), ("n8192_R40", (8192, 40, {})),
    ("n511_R512", (511, 512, {})), ("n512_R512", (512, 512, {})),
    ("n600_R511", (600, 511, {})), ("n600_R512", (600, 512, {})),
    ("n1023_R8_g2_0", (1023, 8, "split_g2_0")), ("n1024_R8_g2_0", (1024, 8, "split_g2_0")),
    ("n16384_R40", (16384, 40, {})), ("n16385_R40", (16385, 40, {})),
    ("n16390_R5", (16390, 5, {})),          # a few relations, each spanning many 4096-item blocks
])
for _i, (_name, (_n, _R, _env)) in enumerate(D_SHAPES.items()):
    _envname = _env if isinstance(_env, str) else "default"
    _order = "interleaved" if _n > SMALL_MAX_N else "shuffled"
    add_case("D", _name, "rescal", 8, False, _even_counts(_n, _R), _order, _envname)
    if _envname == "default":
        add_case("D", _name, "transr", (8, 8) if _n > 8192 else TRANSR_DIMS[_i % 2][:2], False if _n > 8192 else TRANSR_DIMS[_i % 2][2],
                 _even_counts(_n, _R), _order, "default")
# (the tile kernels group the 2 n triples of both sides: their one-launch grouping ends at n = 8192)
add_case("D", "n8192_R40", "rescal", 8, False, _even_counts(8192, 40), "shuffled", "unfused")
add_case("D", "n8193_R40", "rescal", 8, False, _even_counts(8193, 40), "shuffled", "unfused")
add_case("D", "n8192_R40", "transr", (8, 8), False, _even_counts(8192, 40), "shuffled", "rows0")
add_case("D", "n8193_R40", "transr", (8, 8), False, _even_counts(8193, 40), "shuffled", "rows0")

# G: every step form behind the block-aggregated (n > 16384) and the global-atomic (R > 4096) grouping
G_SHAPES = collections.OrderedDict([("lds_n16390_R5", _even_counts(16390, 5)), ("atomic_R4097", scan_counts(4097))])
for _name, _counts in G_SHAPES.items():
    for _envname in distinct_envs("rescal", sum(_counts), len(_counts), 8):
        if _envname != "default":
            add_case("G", _name, "rescal", 8, False, _counts, "interleaved", _envname)
    add_case("G", _name, "rescal", 20, False, _counts, "interleaved", "default")       # k_rescal_g2 (k >= 20)
    for _envname in ("rows0", "g0"):
        add_case("G", _name, "transr", (8, 8), False, _counts, "interleaved", _envname)

GPU_KEYS = list(CASES)

# E: grouped ranks -- test triples per relation (R = 8: tests/test_hip_rank_edges.py), one empty relation at each end
E_RANK_COUNTS = (0, 1, 15, 16, 17, 33, 2, 0)


def rank_queries(rng, counts, E):
    """int64 [n, 3] queries with counts[r] triples of relation r, (h, r) and (r, t) pairwise distinct, in shuffled order."""
    rows = []
    for rel, c in enumerate(counts):
        assert c <= E
        rows += list(zip(rng.permutation(E)[:c].tolist(), [rel] * c, rng.permutation(E)[:c].tolist()))
    q = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    return np.ascontiguousarray(q[rng.permutation(len(q))])


# --------------------------------------------------------------------------------------------------------------- reachable cells
SWEEP_N = (1, 16, 17, 64, 65, 129, 300, 511, 512, 600, 721, 1023, 1024, 4096, 4097, 6000, 8191, 8192, 8193, 16384, 16385, 20000)
SWEEP_R = (1, 5, 8, 14, 40, 300, 511, 512, 1025, 3055, 3056, 4096, 4097)


def reachable_cells():
    """{(model, grouping form, step form)} over a sweep of (n, R), both hidden-size classes and every switch set: what plan() declares
    reachable by the project's own switches."""
    out = set()
    for n in SWEEP_N:
        for R in SWEEP_R:
            for k in (6, 8, 20):
                for env in RESCAL_ENVS.values():
                    p = plan("rescal", n, R, k, env)
                    out.add(("rescal", p.grouping, p.step))
            for env in TRANSR_ENVS.values():
                for dims in ((8, 12), (6, 8)):
                    p = plan("transr", n, R, dims, env)
                    out.add(("transr", p.grouping, p.step))
    return out


def covered_cells(cls=None):
    out = set()
    for c in CASES.values():
        if cls is None or c.cls == cls:
            p = case_plan(c)
            out.add((c.model, p.grouping, p.step))
    return out


# --------------------------------------------------------------------------------------------------------------- float64 side
def hp_of(c):
    if c.model == "rescal":
        return dict(hidden_size=c.dims, margin=1.0, neg_rate=1)
    return dict(ent_hidden_size=c.dims[0], rel_hidden_size=c.dims[1], l1_flag=bool(c.l1), margin=1.0)


def _shape_kw(c):
    return {k: v for k, v in hp_of(c).items() if k in ("hidden_size", "ent_hidden_size", "rel_hidden_size")}


@functools.lru_cache(maxsize=None)
def batch_of(counts, seed, order):
    b = composition(counts, seed, order)
    for a in b[:6]:
        a.setflags(write=False)
    return b


def tables(c, table_seed):
    """Tables of a case: kge_oracle.init_params on a seed made of the case's shape (not of its order or switches: the same tables for
    every form of one composition) and table_seed."""
    b = batch_of(c.counts, c.seed, "sorted")
    word = zlib.crc32(("%s/%r/%r/%r" % (c.model, c.dims, c.l1, c.counts)).encode())
    return ko.init_params(c.model, np.random.default_rng((word, table_seed)), tot_entity=b.E, tot_relation=b.R, **_shape_kw(c))


def transr_l1_residual(P, h, r, t):
    """The L1 residual u = (h^ M_r)^ + r^ - (t^ M_r)^ of TransR in float64 (its signs are the gradient), [n, d_r]."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    eh, et, rl = P["ent_embeddings"][h], P["ent_embeddings"][t], P["rel_embeddings"][r]
    M = P["rel_matrix"][r].reshape(len(r), eh.shape[1], rl.shape[1])
    hh, th = ko._normalize(eh)[0], ko._normalize(et)[0]
    a, c_ = np.einsum("na,nab->nb", hh, M), np.einsum("na,nab->nb", th, M)
    return ko._trans_tail(a, rl, c_, True)[1][6]


def ambiguous(c, P, batch):
    """Pairs of the float64 run within NEAR_MARGIN of the margin, plus (L1 TransR) pairs with a residual component within NEAR_ZERO of 0."""
    hp = hp_of(c)
    ph, pr, pt, nh, nr, nt = batch[:6]
    Pn = ko.rescal_normalize_tables(P, np.float64) if c.model == "rescal" else P
    pos = ko.score(c.model, Pn, ph, pr, pt, dtype=np.float64, **hp)
    neg = ko.score(c.model, Pn, nh, nr, nt, dtype=np.float64, **hp)
    amb = np.abs(pos + hp["margin"] - neg) < sb.NEAR_MARGIN
    if c.model == "transr" and c.l1:
        for h, r, t in ((ph, pr, pt), (nh, nr, nt)):
            amb |= (np.abs(transr_l1_residual(P, h, r, t)) < sb.NEAR_ZERO).any(1)
    return int(amb.sum())


@functools.lru_cache(maxsize=None)
def _table_seed(model, dims, l1, counts, seed):
    c = Case("", "", model, dims, l1, counts, "sorted", "default", {}, seed)
    batch = batch_of(counts, seed, "sorted")
    for s in range(256):
        if ambiguous(c, tables(c, s), batch) == 0:
            return s
    raise AssertionError("no table seed without an ambiguous pair: %s %r %r" % (model, dims, counts[:8]))


def table_seed(c):
    """The first table seed whose float64 run of the case's pairs has no ambiguous pair (the set of pairs does not depend on the order)."""
    return _table_seed(c.model, c.dims, c.l1, c.counts, c.seed)


Ref = collections.namedtuple("Ref", "batch P hp loss G64 cnt a allow")


@functools.lru_cache(maxsize=8)
def _reference(model, dims, l1, counts, seed, order):
    c = Case("", "", model, dims, l1, counts, order, "default", {}, seed)
    b = batch_of(counts, seed, order)
    batch = tuple(b[:6])
    hp = hp_of(c)
    P = tables(c, table_seed(c))
    G64, scores, cnt, side_of, a, ctx = sb.hub_bounds(model, P, batch, hp, b.E, b.R)
    allow, n_amb = sb.ambiguity_allowance(model, P, scores, batch, hp, ctx)
    widen = sb.normalisation_allowance(model, ko.rescal_normalize_tables(P, np.float64) if model == "rescal" else P, batch, hp)
    # the seeds were chosen so: nothing is excused, and at these widths (no normalised vector of length 1) nothing is widened either
    assert n_amb == 0 and all(not v.any() for v in allow.values()) and all(not v.any() for v in widen.values()), (model, dims, n_amb)
    if model == "transr" and l1:
        assert ambiguous(c, P, batch) == 0
    loss = float(ko.train_step_grads(model, P, batch, dtype=np.float64, **hp)[0])
    return Ref(b, P, hp, loss, G64, cnt, a, allow)


def reference(c):
    """The float64 side of a case: gradient, loss and the bar's terms (the allowance asserted to be exactly zero)."""
    return _reference(c.model, c.dims, c.l1, c.counts, c.seed, c.order)


def compare(key, ref, got, after=None):
    """Hold `got` (per-table gradients) to the bar of tests/step_bar.py -> (largest deviation, largest deviation / tolerance)."""
    worst, ratio = 0.0, 0.0
    for k, g in ref.G64.items():
        assert not ref.allow[k].any(), (key, k)
        tol = sb.tolerance(g, ref.cnt[k], ref.a[k], None if after is None else after[k], 0.0)
        err = np.abs(np.asarray(got[k], np.float64) - g)
        bad = err > tol
        if bad.any():
            rows = np.flatnonzero(bad.reshape(len(g), -1).any(1))
            i = np.unravel_index(np.argmax(np.where(bad, err / tol, 0)), g.shape)
            raise AssertionError("%s %s: %d rows off (first %s); worst %s: got %.9g want %.9g tol %.3g c_r %d a_r %.4g"
                                 % (key, k, len(rows), rows[:8].tolist(), i, np.asarray(got[k])[i], g[i], tol[i], ref.cnt[k][i[0]], ref.a[k][i]))
        worst, ratio = max(worst, float(err.max())), max(ratio, float((err / tol).max()))
    return worst, ratio


def gradient_of(c, before, after):
    """The step's gradient at lr = 1: before - after; RESCAL renormalises both tables before its forward (in place), so there it is
    rescal_normalize_tables(before) - after."""
    start = ko.rescal_normalize_tables(before, np.float64) if c.model == "rescal" else before
    return {k: np.asarray(start[k], np.float64) - np.asarray(after[k], np.float64) for k in before}
