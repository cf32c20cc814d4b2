"""The relation-grouped training steps of RESCAL and TransR at their group, tile and scan edges, against float64.

Every step form behind the device-side grouping by relation (csrc/kge_relgroup.h; csrc/kge_dense.hip, kge_rescal_slab.hip,
kge_transr.hip, kge_transr_rows.hip) indexes its work by offsets / tile_off / tile_rel / perm.  The failures of such code -- a
dropped last pair of a relation, a tile attributed to the neighbouring relation, a carry lost between scan passes, a padding lane of
the bitonic sort leaking into perm -- each move a few rows of the gradient by a whole term; a random batch may never produce them.
tests/relgroup_edges_ref.py builds batches whose per-relation counts, relation counts and pair counts sit on every threshold of the
sources, and restates the dispatch (plan()) so that each case names the kernels it is meant to reach.

Method (that of tests/test_hip_skew.py and tests/test_hip_width_edges.py): Trainer(use_graph=False), one SGD step with lr = 1
through train_model_epoch(0), so that before - after is the step's gradient (RESCAL: rescal_normalize_tables(before) - after).  The
generator's sampler is replaced by one that hands out the case's composition as it stands (the Trainer's own generator orders every
batch by relation and corrupts by position, which would undo the orders and the compositions these cases are about); everything
behind it -- the shared relation buffer, the step, the optimiser -- is the Trainer's.  The gradient is held per element to
kge_oracle.train_step_grads in float64 under the bar of tests/step_bar.py, unchanged:
    2e-6 + 2e-4 |g64| + c_r 2^-23 a_r + 2^-24 |after|
with NO hinge / L1 allowance: the table seeds were chosen on the CPU (relgroup_edges_ref.table_seed) so that no pair of the float64
run lies within NEAR_MARGIN of the margin and no L1 TransR residual within NEAR_ZERO of zero, and relgroup_edges_ref.reference
asserts that the allowance (and the normalisation allowance) is exactly zero.  The loss is held at rtol 2e-5.  Where the Trainer or
the library reports the form taken (step_path(), kge_rescal_pair_step_ok, kge_rescal_stage_ok, _rescal_stage, rescal_reproducible)
that report is asserted against plan().

What did not hold as first written down, found while building the cases:
  * counts cycling through (0, 1, 2, 17) have mean 5, so the scan cases have n = 5 R (2.4 R above R = 2048), not 3 R / 2;
  * the LDS bound of the sorted grouping binds only where the split rule is switched off (KGE_RESCAL_SPLIT_MIN);
  * at k = 8 and 12 the 16-byte gather kernel k_rescal_g2 is never launched (launch_rescal_g asks for k >= 20): the g2_ok RULE
    applies there, the dword k_rescal_g runs; k = 20 cases reach k_rescal_g2;
  * the staged step equals itself bit for bit across presentations of one batch only where every relation's own pairs keep their
    relative order (sorting by pair index restores exactly that): "shuffled" interleaves the relations and keeps it.

Measured on an MI355X: profiles/r29_relgroup_edges.txt."""
import numpy as np
import pytest

import kge_oracle as ko
import relgroup_edges_ref as rg
import step_bar as sb

gpu = pytest.mark.gpu
REPORT = "relgroup_edges_deviation"


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    for k in rg.SWITCHES + ("KGE_EVAL_GEMM",):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------------ CPU: composition, grouping_ref
def test_composition_delivers_the_counts_in_every_order():
    for counts in list(rg.A_COUNTS.values()) + list(rg.B_COUNTS.values()) + [rg.scan_counts(257), rg.scan_counts(300, 16385)]:
        R, n = len(counts), sum(counts)
        sets = []
        for order in rg.ORDERS:
            b = rg.composition(counts, 3, order)
            assert (b.E, b.R, b.counts, b.order) == (rg.entity_count(n), R, tuple(counts), order)
            assert all(len(x) == n and x.dtype == np.int64 for x in b[:6]) and b.nr is not None and np.array_equal(b.pr, b.nr)
            assert np.bincount(b.pr, minlength=R).tolist() == list(counts)
            assert all(0 <= x.min() and x.max() < b.E for x in (b.ph, b.pt, b.nh, b.nt))
            assert ((b.ph != b.nh) ^ (b.pt != b.nt)).all()                      # a negative differs on exactly one side
            assert len({(h, r, t) for h, r, t in zip(b.ph.tolist(), b.pr.tolist(), b.pt.tolist())}) == n
            sets.append(sorted(zip(*[x.tolist() for x in b[:6]])))
            offsets, tile_off, members, tile_rel = rg.grouping_ref(b.pr, R, 16)
            assert offsets[R] == n and np.diff(offsets).tolist() == list(counts)
            assert np.diff(tile_off).tolist() == [-(-c // 16) for c in counts] and len(tile_rel) == tile_off[R]
            assert all((b.pr[members[rel]] == rel).all() and len(members[rel]) == counts[rel] for rel in range(R))
            for rel in range(R):                                                # a tile names the relation whose range it lies in
                assert (tile_rel[tile_off[rel]:tile_off[rel + 1]] == rel).all()
            if order == "sorted":
                assert (np.diff(b.pr) >= 0).all()
                if n >= 64:     # rows repeat inside a tile (neighbours of one relation share a head or a tail) and across tiles
                    same = int((np.diff(b.pr) == 0).sum())
                    assert (b.ph[1:] == b.ph[:-1]).sum() >= same // 6 and (b.pt[1:] == b.pt[:-1]).sum() >= same // 9
                    assert np.bincount(np.concatenate([b.ph, b.pt, b.nh, b.nt]), minlength=b.E).max() >= 8
            if order == "interleaved" and n > rg.GROUP_ITEMS:                   # every block sees every relation that still has pairs
                for lo in range(0, n, rg.GROUP_ITEMS):
                    left = np.bincount(b.pr[lo:], minlength=R) > 0
                    here = np.bincount(b.pr[lo:lo + rg.GROUP_ITEMS], minlength=R) > 0
                    assert here[left].all() or (n - lo) < rg.GROUP_ITEMS
        assert sets[0] == sets[1] == sets[2]
    # "shuffled" keeps every relation's own pairs in drawing order
    a, b = rg.composition(rg.B_COUNTS["sortable"], 0, "sorted"), rg.composition(rg.B_COUNTS["sortable"], 0, "shuffled")
    assert not np.array_equal(a.pr, b.pr)
    for rel in range(a.R):
        assert all(np.array_equal(x[a.pr == rel], y[b.pr == rel]) for x, y in zip(a[:6], b[:6]))


def test_scan_counts_keep_both_sides_of_every_pass_boundary_busy():
    for R in rg.SCAN_R:
        for n_min in (None, 16385):
            c = np.asarray(rg.scan_counts(R, n_min))
            assert len(c) == R and (c.sum() >= n_min if n_min else c.sum() <= rg.SMALL_MAX_N) and (c == 0).sum() >= R // 4 - 1
            for width in (rg.SCAN, rg.SMALL_SCAN):
                for b in range(width, R, width):
                    assert c[b - 1] > 0 and c[b] > 0, (R, b)
                    for tile in (16, 32, 64):       # both carries differ from their neighbours': the carried sums are non-trivial
                        assert c[:b].sum() > 0 and (-(-c[:b] // tile)).sum() != c[:b].sum()


# ------------------------------------------------------------------------------------------------------ CPU: plan
def _p(model, n, R, k, envname="default"):
    return rg.plan(model, n, R, k, rg.ENVS[model][envname])


def test_plan_agrees_with_itself_on_both_sides_of_every_threshold():
    # grouping forms (group_by_relation_split)
    assert [rg.grouping_form(n, R) for n, R in ((16384, 4096), (16385, 4096), (16384, 4097), (16385, 4097), (1, 1))] == \
        ["small", "lds", "atomic", "atomic", "small"]
    assert rg.grouping_form(8192, 5, zero_n=16384) == "small" and rg.grouping_form(8193 * 2, 5, zero_n=8193 * 2) == "lds"
    # RESCAL step forms: pair_split at 8191 / 8192, at 511 / 512 pairs with R = 512, at R = 511 / 512 with n = 600
    assert [_p("rescal", n, 40, 8).step for n in (8191, 8192)] == ["slab", "rows+g"]
    assert [_p("rescal", n, 512, 8).step for n in (511, 512)] == ["slab", "rows+g"]
    assert [_p("rescal", 600, R, 8).step for R in (511, 512)] == ["slab", "rows+g"]
    # gemm_g: g2_ok, or n >= 128 R
    assert [_p("rescal", n, 8, 8, "split_g2_0").step for n in (1023, 1024)] == ["rows+gm", "rows+g"]
    assert [_p("rescal", n, 8, 6, "split").step for n in (1023, 1024)] == ["rows+gm", "rows+g"]
    # the 16-byte gather needs k >= 20
    assert [_p("rescal", 721, 14, k, "split").kernels[-1] for k in (8, 12, 16, 20)] == ["k_rescal_g"] * 3 + ["k_rescal_g2"]
    assert _p("rescal", 721, 14, 6, "slab0").kernels == ("k_rescal_pair<2>",) and _p("rescal", 721, 14, 8, "slab0").kernels == ("k_rescal_pair<4>",)
    assert _p("rescal", 721, 14, 8, "split_rows0").kernels == ("k_rescal_pair<4>", "k_rescal_pair_gm")
    assert _p("rescal", 721, 14, 8, "split_rows0_g1").step == "pair+gm"       # gemm_g needs rows
    # grouping behind the step forms: 16384 / 16385; R = 4096 / 4097; the tile kernels group 2 n triples
    assert [_p("rescal", n, 40, 8).grouping for n in (16384, 16385)] == ["small", "lds"]
    assert [_p("transr", n, 40, (8, 8)).grouping for n in (16384, 16385)] == ["small", "lds"]
    assert [_p("rescal", 9000, R, 8).grouping for R in (4096, 4097)] == ["small", "atomic"]
    assert [_p("rescal", n, 40, 8, "unfused").grouping for n in (8192, 8193)] == ["small", "lds"]
    assert [_p("transr", n, 40, (8, 8), "rows0").grouping for n in (8192, 8193)] == ["small", "lds"]
    assert [_p("rescal", 9000, R, 8).scan_passes for R in (1024, 1025, 4096, 4097)] == [1, 2, 4, 17]
    assert [_p("rescal", 16385, R, 8).scan_passes for R in (255, 256, 257)] == [1, 1, 2]
    # the staged form: k % 4, n <= 4096, the LDS bound, the slab form
    assert [_p("rescal", n, 40, 8, "staged").staged for n in (4096, 4097)] == [True, False]
    assert [_p("rescal", n, R, 12, "staged_nosplit").staged for n, R in rg.B_LDS] == [True, False]
    assert not any(_p("rescal", n, R, 12, "staged").staged for n, R in rg.B_LDS)      # (the default rule splits there)
    assert [(3 * R + 2 * n + 2) * 4 <= rg.STAGE_LDS for n, R in rg.B_LDS] == [True, False]
    assert not _p("rescal", 721, 14, 6, "staged").staged and _p("rescal", 721, 14, 8, "staged").grouping == "small_sorted"
    assert not _p("rescal", 721, 14, 8, "default").staged       # (tables below 32 MB: not fused, so nothing is staged by default)
    # TransR
    assert _p("transr", 721, 14, (8, 12)).kernels == ("k_transr_rows", "k_transr_g2") and _p("transr", 721, 14, (8, 12), "g0").kernels[-1] == "k_transr_g"
    assert _p("transr", 721, 14, (8, 12), "rows1") == _p("transr", 721, 14, (8, 12), "rows2") == _p("transr", 721, 14, (8, 12))
    assert _p("transr", 721, 14, (8, 12), "rows0").step == "tiles32" and _p("transr", 721, 14, (8, 12), "rows0").items == 1442


def test_case_lists_have_no_empty_cell():
    """Every (model, grouping form, step form) plan() declares reachable has a case; every A composition runs every distinct launch its
    (n, R) can reach by the switches; B, C, D and G hold the cells and the shapes the thresholds ask for."""
    assert rg.reachable_cells() <= rg.covered_cells(), sorted(rg.reachable_cells() - rg.covered_cells())
    by = {}
    for c in rg.CASES.values():
        by.setdefault((c.cls, c.model, c.counts, c.dims), set()).add(c.envname)
    for i, (name, counts) in enumerate(rg.A_COUNTS.items()):
        n, R = sum(counts), len(counts)
        ks = ((8, 12)[i % 2],) + ((6, 20) if name == "edges" else ())
        assert set(rg.distinct_envs("rescal", n, R, ks[0])) == by[("A", "rescal", tuple(counts), ks[0])], name
        steps = {rg.plan("rescal", n, R, k, rg.RESCAL_ENVS[e]).step for k in ks for e in by[("A", "rescal", tuple(counts), k)]}
        want = {"slab", "slab_staged", "pair", "pair+gm", "rows+g", "rows+gm", "tiles32"} | ({"rows+g2"} if name == "edges" else set())
        assert steps == want, (name, steps)
        assert by[("A", "transr", tuple(counts), rg.TRANSR_DIMS[i % 2][:2])] == set(rg.TRANSR_ENVS), name
    kernels = {k for c in rg.CASES.values() if c.cls == "A" for k in rg.case_plan(c).kernels}
    assert kernels >= {"k_rescal<0>", "k_rescal<1>", "k_rescal_gm", "k_rescal_pair<2>", "k_rescal_pair<4>", "k_rescal_pair_gm", "k_rescal_rows",
                       "k_rescal_g", "k_rescal_g2", "rescal_slab", "k_transr<0>", "k_transr<1>", "k_transr_rows", "k_transr_g", "k_transr_g2"}
    # A: every per-relation count of the issue's list is held by some relation, next to an empty one, at both ends and in the middle
    assert set(rg.TILE_EDGE_COUNTS) == {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129}
    assert rg.A_COUNTS["edges"][0] == 0 and rg.A_COUNTS["edges_rev"][-1] == 0 and (0, 0) == rg.A_COUNTS["edges_gap"][7:9]
    assert rg.group_max_tiles_ok((1,) * 300, 16)
    # B
    cells = {(c.model,) + rg.case_plan(c)[:1] + (rg.case_plan(c).step,) for c in rg.CASES.values() if c.cls == "B"}
    assert cells == {("rescal", "small_sorted", "slab_staged"), ("rescal", "small", "slab")}
    assert {1, 2, 63, 64} <= set(rg.B_COUNTS["sortable"]) and max(rg.B_COUNTS["sortable"]) == 64 and max(rg.B_COUNTS["one_65"]) == 65
    # C: every R of the list through both models, below and above n = 16384; R = 4097 is the global-atomic grouping
    for model in ("rescal", "transr"):
        got = {(len(c.counts), rg.case_plan(c).grouping) for c in rg.CASES.values() if c.cls == "C" and c.model == model}
        assert got == {(R, "small" if R <= 4096 else "atomic") for R in rg.SCAN_R} | {(R, "lds" if R <= 4096 else "atomic") for R in rg.SCAN_R}
    assert all(rg.case_plan(c).grouping == "atomic" for c in rg.CASES.values() if c.cls == "C" and len(c.counts) == 4097)
    # D: both sides of every threshold
    shapes = {(c.model, sum(c.counts), len(c.counts), c.envname) for c in rg.CASES.values() if c.cls == "D"}
    for n, R in ((8191, 40), (8192, 40), (511, 512), (512, 512), (600, 511), (600, 512), (16384, 40), (16385, 40), (16390, 5)):
        assert ("rescal", n, R, "default") in shapes and ("transr", n, R, "default") in shapes
    assert {("rescal", 1023, 8, "split_g2_0"), ("rescal", 1024, 8, "split_g2_0"), ("rescal", 8192, 40, "unfused"), ("rescal", 8193, 40, "unfused"),
            ("transr", 8192, 40, "rows0"), ("transr", 8193, 40, "rows0")} <= shapes
    # G: both large grouping forms under every step form
    for form in ("lds", "atomic"):
        assert {s for m, g, s in rg.covered_cells("G") | rg.covered_cells("D") | rg.covered_cells("C") if m == "rescal" and g == form} == \
            {"pair", "pair+gm", "rows+g", "rows+g2", "rows+gm", "tiles32"}
        assert {s for m, g, s in rg.covered_cells("G") | rg.covered_cells("C") if m == "transr" and g == form} == {"rows+g", "rows+g2", "tiles32"}


def _unique_references(max_n):
    seen, out = set(), []
    for c in rg.CASES.values():
        sig = (c.model, c.dims, c.l1, c.counts, c.seed, c.order)
        if sig not in seen and sum(c.counts) <= max_n:
            seen.add(sig)
            out.append(c)
    return out


def test_reference_fp32_meets_the_bar_with_no_allowance():
    """The fp32 numpy oracle meets the bar against the float64 one on the cases' inputs with no allowance at all (reference() asserts the
    allowance is zero): the inputs and the bar admit a correct fp32 implementation.  (Compositions up to 1100 pairs: the larger ones
    are drawn and seeded the same way.)"""
    for c in _unique_references(1100):
        ref = rg.reference(c)
        loss32, G32, _s, _P = ko.train_step_grads(c.model, ref.P, tuple(ref.batch[:6]), dtype=np.float32, **ref.hp)
        rg.compare(c.key, ref, G32)
        assert np.isclose(float(loss32), ref.loss, rtol=2e-5), (c.key, float(loss32), ref.loss)


MISTAKE_CASES = {"drop_last": ("A/rescal/edges/k8/shuffled/default", 16, False),
                 "lost_carry": ("C/rescal/scan_R1025/k12/shuffled/default", 64, False),
                 "tile_rel_at_1": ("A/transr/edges/d8x12/shuffled/default", 16, False),
                 "padding_zero": ("B/rescal/sortable/k8/shuffled/staged", 64, True),
                 "full_tile": ("A/rescal/edges_rev/k12/shuffled/default", 64, False)}


@pytest.mark.parametrize("mistake", rg.MISTAKES)
def test_the_bar_sees_each_grouping_mistake(mistake):
    """What the cases are for, on the CPU: a value-level model of the grouping with one deliberate mistake (relgroup_edges_ref.
    consumed_pairs) hands the float64 oracle the pairs a step would then consume; that gradient misses the bar of the case, while the
    same model without the mistake consumes the batch as it is.  (On the device each of these mistakes but the first also leaves
    index entries that nothing wrote, so they are not run there.)"""
    key, tile, sort = MISTAKE_CASES[mistake]
    c = rg.CASES[key]
    ref = rg.reference(c)
    batch = [np.asarray(x) for x in ref.batch[:6]]
    right = rg.consumed_pairs(batch[1], ref.batch.R, tile, None, sort=sort)
    assert sorted(right) == sorted(zip(batch[1].tolist(), range(len(batch[1]))))
    wrong = rg.consumed_pairs(batch[1], ref.batch.R, tile, mistake, sort=sort)
    assert sorted(wrong) != sorted(right)
    rel, at = (np.asarray(x, dtype=np.int64) for x in zip(*wrong))
    taken = (batch[0][at], rel, batch[2][at], batch[3][at], rel, batch[5][at])
    _l, G, _s, _P = ko.train_step_grads(c.model, ref.P, taken, dtype=np.float64, **ref.hp)
    with pytest.raises(AssertionError, match="rows off"):
        rg.compare(key, ref, G)


# ------------------------------------------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def hip():
    import torch
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


class _Composed:
    """The generator's backend with the sampler replaced: sample_batch hands out the case's composition (device tensors)."""

    def __init__(self, K, batch):
        self._K, self._batch, self.handed = K, batch, 0

    def __getattr__(self, name):
        return getattr(self._K, name)

    def sample_batch(self, triples, perm, start, n_pos, neg_rate, *a, **kw):
        assert (start, n_pos, neg_rate) == (0, self._batch[0].numel(), 1), (start, n_pos, neg_rate)
        self.handed += 1
        return [x.clone() for x in self._batch]


def _trainer(hip, c, ref, monkeypatch):
    import torch
    from pykg2vec_amd.trainer import Trainer
    b = ref.batch
    n = len(b.ph)
    for k in rg.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    train = np.stack([b.ph, b.pr, b.pt], 1)
    cfg = hip.make_config(b.E, b.R, ref.hp, train, train[:8], train[:8], optimizer="sgd", lr=1.0, batch_size=n)
    cfg.tot_train_triples = n           # one step per epoch
    m = hip.model_from_params(c.model, ref.P, ref.hp, b.E, b.R, train=train)
    tr = Trainer(m, cfg, use_graph=False)
    tr.build_model()
    gen = tr.generator = tr._new_generator()
    gen.perm = torch.arange(n, dtype=gen.perm.dtype, device=gen.perm.device)      # the batch is the train split as it stands
    gen.K = _Composed(gen.K, [hip.dev(x) for x in b[:6]])
    return tr, m


def _tables(hip, m):
    return {k[:-len(".weight")]: p.detach().cpu().numpy().copy() for k, p in hip.table_parameters(m)}


def _step(hip, c, monkeypatch):
    """One step of a case -> (trainer, before, after, flat parameters, loss), the reports of the form taken asserted on the way."""
    from pykg2vec_amd import kernels as K
    p, ref = rg.case_plan(c), rg.reference(c)
    n, R = len(ref.batch.ph), ref.batch.R
    tr, m = _trainer(hip, c, ref, monkeypatch)
    assert tr.step_path(1) == "generic", (c.key, tr.step_path(1))
    if c.model == "rescal":
        desc = K.model_desc(m)
        assert K.rescal_pair_step_ok(desc, n) == (c.dims % 2 == 0 and c.dims <= 256), c.key
        assert K.rescal_stage_ok(desc, n) == rg.rescal_stage_ok(n, R, c.dims, c.env), (c.key, n, R)
    before = _tables(hip, m)
    after, flat, _state, loss = sb.one_step(hip, tr, m)
    assert tr.generator.K.handed == 1, c.key
    if c.model == "rescal":
        assert (getattr(tr, "_rescal_stage", None) is not None) == p.staged, (c.key, p)
        if p.staged:
            assert tr.rescal_reproducible is (max(c.counts) <= rg.SLAB_CHUNK), (c.key, tr.rescal_reproducible)
    return tr, ref, before, after, flat, loss


@gpu
@pytest.mark.parametrize("key", rg.GPU_KEYS)
def test_grouped_step_at_its_edges_matches_float64(hip, monkeypatch, key):
    c = rg.CASES[key]
    p = rg.case_plan(c)
    tr, ref, before, after, _flat, loss = _step(hip, c, monkeypatch)
    got = rg.gradient_of(c, before, after)
    print("MEASURED", key, p.grouping, p.step, "loss", loss, ref.loss)
    worst, ratio = None, None
    try:
        worst, ratio = rg.compare(key, ref, got, after)
    finally:
        print("MEASURED", key, "max_abs", worst, "of_tolerance", ratio)
    assert np.isclose(loss, ref.loss, rtol=2e-5), (key, loss, ref.loss)
    form = "%s/%s/%s" % (c.model, p.grouping, p.step)
    hip.record_max(REPORT, form + "/max_abs", worst)
    hip.record_max(REPORT, form + "/of_tolerance", ratio)
    hip.record_max(REPORT, form + "/loss_rel", abs(loss - ref.loss) / abs(ref.loss))


@gpu
def test_sorted_grouping_makes_the_staged_step_bit_reproducible(hip, monkeypatch):
    """Relations of 2 .. 64 pairs are sorted by pair index: the staged step is the same bit for bit on two runs, and on the same pairs
    presented in relation order (every relation's own pairs keep their relative order in both presentations, so sorting by pair index
    arrives at one grouped order).  rescal_reproducible says so; with one relation of 65 pairs it says False."""
    import torch
    flats = {}
    for order in ("shuffled", "shuffled", "sorted"):
        c = rg.CASES["B/rescal/sortable/k8/%s/staged" % order]
        assert rg.case_plan(c).grouping == "small_sorted"
        tr, _ref, _b, _a, flat, _loss = _step(hip, c, monkeypatch)
        assert tr.rescal_reproducible is True
        flats.setdefault(order, []).append(flat)
    assert torch.equal(flats["shuffled"][0], flats["shuffled"][1]), "two runs of the staged step differ"
    assert torch.equal(flats["shuffled"][0], flats["sorted"][0]), "the staged step depends on how the relations are interleaved"
    tr, *_ = _step(hip, rg.CASES["B/rescal/one_65/k8/shuffled/staged"], monkeypatch)
    assert tr.rescal_reproducible is False


@gpu
def test_staged_form_is_refused_beyond_its_bounds_and_the_step_falls_back(hip, monkeypatch):
    """n = 4097 and the (n, R) beyond the LDS bound: kge_rescal_stage_ok says no, the Trainer stages nothing and runs the plain pair step
    (whose result test_grouped_step_at_its_edges_matches_float64 holds to the bar); asking the library for the staged form anyway is an
    error with a message, not a launch."""
    import torch
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd._lib import KgeHipError
    for key in ("B/rescal/n4097/k8/shuffled/staged", "B/rescal/lds_n%d_R%d/k12/shuffled/staged_nosplit" % rg.B_LDS[1]):
        c = rg.CASES[key]
        ref = rg.reference(c)
        tr, m = _trainer(hip, c, ref, monkeypatch)
        n = len(ref.batch.ph)
        assert not K.rescal_stage_ok(K.model_desc(m), n) and tr._rescal_stage_for(n) is None and getattr(tr, "_rescal_stage", None) is None
        ent = tr.flat.views[0]
        st = K.RescalStage(ent.shape[0], n, ent.shape[1], ent.device)
        touched = torch.zeros((ent.shape[0] + 31) // 32, dtype=torch.int32, device=ent.device)
        ph, pr, pt, nh, _nr, nt = [hip.dev(x) for x in ref.batch[:6]]
        with pytest.raises(KgeHipError, match="staged form takes"):
            K.rescal_pair_step_staged(tr._desc, ph, pr, pt, nh, nt, 1.0, tr.loss_buf, touched, st)


# ------------------------------------------------------------------------------------------------------ E: grouped ranks
@gpu
@pytest.mark.parametrize("family", ["transr_l1", "transr_l2"])
def test_grouped_ranks_at_relation_group_edges(family):
    """kge_eval_ranks_grouped (TransR: every test triple goes through the per-relation candidate tables) with 0, 1, 15, 16, 17 and 33
    test triples per relation, an empty relation at each end: raw rank, filtered rank and ties equal the numpy counts over the model's
    own rows (tests/rank_edges_ref.py), no tolerance."""
    import torch
    import rank_edges_ref as ref
    import test_hip_rank_edges as tre
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert len(rg.E_RANK_COUNTS) == tre.R and rg.E_RANK_COUNTS[0] == rg.E_RANK_COUNTS[-1] == 0
    for E, width in ((65, 6), (257, 32)):
        rng = np.random.default_rng(2900 + E)
        q = rg.rank_queries(rng, rg.E_RANK_COUNTS, E)
        assert np.bincount(q[:, 1], minlength=tre.R).tolist() == list(rg.E_RANK_COUNTS)
        known = ref.known_triples(rng, q, E, tre.R)
        env = tre.Env(family, width, E, q, known)
        ranks, ties, grouped = env.rank_all()
        assert grouped, family
        env.check_counts(ranks, ties, tag="grouped E=%d" % E)
        first = env.eval_ranks()                        # ... and the per-relation calls of kge_eval_ranks give the same
        env.check_counts(*first, tag="per relation E=%d" % E)
        assert np.array_equal(ranks, first[0]) and np.array_equal(ties, first[1])
