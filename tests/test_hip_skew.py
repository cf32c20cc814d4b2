"""Every step path on heavy-tailed ids (golden_util.skewed_triples: Zipf(0.9) entities, Zipf(1.0) relations) against a float64
restatement of the same batch.  Uniform ids give an entity row a handful of incidences per batch; here hub rows collect hundreds to
thousands, which is what runs the multi-item split of the owner index, the global partial sums and finishing launch of k_pull_step,
the bucket-overflow walks, the staged RotatE step's relation-chunk pre-reduction and the RESCAL slab step's multi-chunk relation
gradients.

One SGD step with lr = 1 through train_model_epoch turns a step into its own gradient (p_before - p_after).  It is held, per element,
to the float64 oracle gradient of the batch kge_sample_batch restates, with a bar per row r of c_r incidences:
    2e-6 + 2e-4 |g64| + c_r 2^-23 a_r        (the uniform tests' atol 2e-6 / rtol 2e-4, plus the fp32 summation bound)
where a_r = sum over the row's incidences of |that incidence's contribution| (float64; fp32 sums of c_r terms in any order stay inside
it).  The a_r term is needed on short rows too: TransE's per-incidence contributions pass the normalisation backward and are ~10 for
rows of norm ~0.1, while five of them can cancel to 1e-3 -- the fp32 numpy oracle itself misses atol 2e-6 there.  a_r comes from the
oracle: every incidence is moved onto its own fresh copy of its row, so the dense gradient of the copies is the per-incidence
contributions.  Hub rows (c_r > 8) must exist in every case and their largest deviations are recorded.  The bar itself (the oracle
bounds, the ambiguity allowance, the tolerance line) lives in tests/step_bar.py, shared with tests/test_hip_width_edges.py."""
import numpy as np
import pytest
import torch

import kge_oracle as ko
from golden_util import skewed_triples
from step_bar import NEAR_MARGIN, NEAR_ZERO, tolerance   # noqa: F401  (the bar's constants, as this file has always named them)
from step_bar import ambiguity_allowance as _ambiguity_allowance, hub_bounds as _hub_bounds, one_step as _one_step, sampled as _sampled

pytestmark = pytest.mark.gpu

SHORT_ROW = 8          # rows with more incidences than one work item takes are the hub rows


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def _world(model, E, R, B, shape_kw, seed):
    rng = np.random.default_rng(seed)
    train = skewed_triples(rng, 2 * B + 17, E, R)
    P = ko.init_params(model, rng, tot_entity=E, tot_relation=R, **shape_kw)
    return train, P


def _trainer(hip, model, hp, E, R, B, world, env, monkeypatch, segment=None):
    from pykg2vec_amd.trainer import Trainer
    train, P = world
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    cfg = hip.make_config(E, R, hp, train, train[:8], train[:8], optimizer="sgd", lr=1.0, batch_size=B)
    cfg.tot_train_triples = B           # one step per epoch
    m = hip.model_from_params(model, P, hp, E, R, train=train)
    tr = Trainer(m, cfg, use_graph=False)
    tr.build_model()
    tr.generator = tr._new_generator()
    if segment is not None:
        tr.generator.pull_segment = segment
    return tr, m


def _check(hip, key, model, P, before, after, batch, hp, E, R, n_pairs, flat_grad=None, multi=None):
    """Per-row tolerance comparison of the step's gradient (before - after, or the given one) with the float64 oracle.  `multi`: rows
    (owner-index numbering, relations after the E entities) the index sends through global partial sums -- they must be compared."""
    G64, scores, cnt, side_of, a, ctx = _hub_bounds(model, P, batch, hp, E, R)
    allow, n_amb = _ambiguity_allowance(model, P, scores, batch, hp, ctx)
    hip.record_max("skew_hub_deviation", "%s/ambiguous_pairs" % key, n_amb)
    assert n_amb <= 0.01 * n_pairs, (n_amb, n_pairs)
    worst = 0.0
    for k in G64:
        s = side_of[k]
        got = flat_grad[k] if flat_grad is not None else before[k].astype(np.float64) - after[k].astype(np.float64)
        g = G64[k]
        tol = tolerance(g, cnt[s], a[k], None if after is None else after[k], allow[k])     # tests/step_bar.py
        bad = np.abs(got - g) > tol
        if bad.any():
            rows = np.flatnonzero(bad.reshape(len(g), -1).any(1))
            i = np.unravel_index(np.argmax(np.where(bad, np.abs(got - g) / tol, 0)), g.shape)
            raise AssertionError("%s: %d rows off (first %s); worst %s: got %.9g want %.9g tol %.3g c_r %d a_r %.4g |after| %.4g"
                                 % (k, len(rows), rows[:8].tolist(), i, got[i], g[i], tol[i], cnt[s][i[0]], a[k][i],
                                    0.0 if after is None else abs(after[k][i])))
        # every row is compared; the hub rows' deviations are the ones recorded
        heavy = cnt[s] > SHORT_ROW
        assert heavy.any(), k
        top = int(np.argmax(cnt[s]))
        dev = float(np.abs(got - g)[heavy].max())
        hip.record_max("skew_hub_deviation", "%s/%s" % (key, k), dev)
        hip.record_max("skew_hub_deviation", "%s/%s/top_row_c%d" % (key, k, cnt[s][top]), float(np.abs(got[top] - g[top]).max()))
        hip.record_max("skew_hub_deviation", "%s/%s/of_tolerance" % (key, k), float((np.abs(got - g) / tol)[heavy].max()))
        worst = max(worst, dev)
    # the heaviest rows are where the skew lives
    assert cnt["ent"].max() > 32 and cnt["rel"].max() > 32, (cnt["ent"].max(), cnt["rel"].max())
    if multi is not None:   # ... and at least one of the two heaviest rows is one the index sends through global partial sums
        assert {int(cnt["ent"].argmax()), E + int(cnt["rel"].argmax())} & set(np.asarray(multi).tolist()), "no top row in multi"
    return worst


def _run_case(hip, monkeypatch, key, model, hp, E, R, B, world, env, path, segment=None, pointwise=False, neg=1,
              deterministic=True):
    runs = []
    for _ in range(2):
        tr, m = _trainer(hip, model, hp, E, R, B, world, env, monkeypatch, segment)
        assert tr.step_path(1) == path, (tr.step_path(1), path)
        before = {k[:-len(".weight")]: p.detach().cpu().numpy().copy() for k, p in hip.table_parameters(m)}
        batch = _sampled(tr, B, neg, E, pointwise)
        runs.append((tr, before, batch) + _one_step(hip, tr, m))
    (tr, before, batch, after, pa, sa, loss), (_tr2, _b2, batch2, _a2, pb, sb, loss2) = runs
    assert all(np.array_equal(x, y) for x, y in zip(batch, batch2))
    want, _G, _s, _P = ko.train_step_grads(model, before, batch, dtype=np.float64, **hp)
    assert np.isclose(loss, want, rtol=2e-5), (key, loss, float(want))
    hip.record_max("skew_hub_deviation", "%s/loss_rel" % key, abs(loss - want) / abs(want))
    if deterministic:
        assert torch.equal(pa, pb) and (sa is None or torch.equal(sa, sb)), key
    return tr, before, batch, after, pa, pb, sa, sb


def _multi_rows(tr):
    """Rows (entities, then relations after E) of batch 0 that the owner index sends through global partial sums."""
    idx = tr.generator._pull_index
    assert idx is not None
    return idx.batch(0)[3][:, 0].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- pull (TransE)
E1, R1, B1 = 14951, 1345, 32768     # config C1


@pytest.fixture(scope="module")
def c1_world():
    return _world("transe", E1, R1, B1, dict(hidden_size=100), seed=2101)


@pytest.mark.parametrize("l1,two_phase,segment", [(True, "0", None), (True, "0", 2), (True, "0", 1),
                                                  (True, "1", None), (True, "1", 2), (True, "1", 1),
                                                  (False, "0", None), (False, "0", 2), (False, "0", 1)])
def test_pull_step_on_zipf_ids_matches_float64(hip, monkeypatch, c1_world, l1, two_phase, segment):
    """k_pull_step (one- and two-phase) at C1's size on Zipf ids: hub rows of thousands of incidences cut into items of `segment`
    (default: 8 one-phase, 32 two-phase) summed through global partial slots and the finishing launch."""
    hp = dict(hidden_size=100, l1_flag=l1, margin=1.0)
    env = {"KGE_PULL": "1", "KGE_PULL_DIR": two_phase}
    key = "pull/%s/%s/seg%s" % ("l1" if l1 else "l2", "two_phase" if two_phase == "1" else "one_phase", segment)
    tr, before, batch, after, *_ = _run_case(hip, monkeypatch, key, "transe", hp, E1, R1, B1, c1_world, env, "pull", segment)
    assert (tr._pull.direction is not None) == (two_phase == "1" and l1)
    if segment is not None:
        assert tr.generator._pull_index.segment == segment
    _check(hip, key, "transe", c1_world[1], before, after, batch, hp, E1, R1, B1, multi=_multi_rows(tr))


# ---------------------------------------------------------------------------------------------------------------- own (pointwise)
@pytest.mark.parametrize("model", ["complex", "distmult"])
def test_own_step_on_zipf_ids_matches_float64(hip, monkeypatch, model):
    """The two-phase owner step of DistMult / ComplEx (csrc/kge_own.hip) with hub entity and relation rows."""
    E, R, D, B = 4000, 11, 200, 4096
    world = _world(model, E, R, B, dict(hidden_size=D), seed=2102)
    hp = dict(hidden_size=D, lmbda=1e-3, neg_rate=1)
    env = {"KGE_PW_PULL": "1", "KGE_STAGED": None}
    key = "own/%s" % model
    tr, before, batch, after, *_ = _run_case(hip, monkeypatch, key, model, hp, E, R, B, world, env, "own", pointwise=True)
    _check(hip, key, model, world[1], before, after, batch, hp, E, R, 2 * B, multi=_multi_rows(tr))


# ---------------------------------------------------------------------------------------------------------------- staged RotatE
def test_staged_rotate_step_on_zipf_ids_matches_float64(hip, monkeypatch):
    """The staged RotatE step (csrc/kge_staged.hip) with neg 8: hub entities walk long overflow chains, and the heaviest relation
    carries far more than kRelChunk (16) slots, so its list is pre-reduced in chunks."""
    from pykg2vec_amd.generator import StagedIndex
    E, R, D, B, neg = 2000, 37, 200, 512, 8
    world = _world("rotate", E, R, B, dict(hidden_size=D, margin=6.0), seed=2103)
    hp = dict(hidden_size=D, margin=6.0, neg_rate=neg, alpha=0.5)
    tr, before, batch, after, *_ = _run_case(hip, monkeypatch, "staged/rotate", "rotate", hp, E, R, B, world, {"KGE_STAGED": "1"},
                                             "staged", neg=neg)
    sx = tr.generator._staged_index
    assert sx is not None and sx.max_rel_list > StagedIndex.LONG_LIST and sx.chunks(0) is not None
    pos_rel = np.bincount(batch[1], minlength=R)
    assert pos_rel.max() > StagedIndex.REL_CHUNK
    _check(hip, "staged/rotate", "rotate", world[1], before, after, batch, hp, E, R, B * neg)


# ---------------------------------------------------------------------------------------------------------------- transx (TransH)
def test_transh_step_on_zipf_ids_matches_float64(hip, monkeypatch):
    """TransH's two-launch owner step (csrc/kge_pullx.hip) with hub rows across workgroups (partials + finishing launch)."""
    E, R, D, B = 3000, 40, 100, 4096
    world = _world("transh", E, R, B, dict(hidden_size=D), seed=2104)
    hp = dict(hidden_size=D, l1_flag=False, margin=1.0)   # (L1 on TransE above; L2 here reaches the projection's backward smoothly)
    tr, before, batch, after, *_ = _run_case(hip, monkeypatch, "transx/transh", "transh", hp, E, R, B, world,
                                             {"KGE_TRANSX_OWN": "1"}, "transx")
    _check(hip, "transx/transh", "transh", world[1], before, after, batch, hp, E, R, B, multi=_multi_rows(tr))


# ---------------------------------------------------------------------------------------------------------------- RESCAL slab
def test_rescal_staged_slab_step_on_zipf_ids_matches_float64(hip, monkeypatch):
    """The staged RESCAL pair step: hub relations span many 64-pair chunks, whose relation-matrix shares meet in float atomics
    (equal to rounding, inside the per-row bound), and the flag that says so is False.  RESCAL renormalises both tables before the
    forward, in place: the step's gradient is rescal_normalize_tables(before) - after (the epoch's last step leaves the tables as the
    optimiser wrote them)."""
    E, R, k, B = 3000, 37, 64, 1024
    world = _world("rescal", E, R, B, dict(hidden_size=k), seed=2105)
    hp = dict(hidden_size=k, margin=1.0, neg_rate=1)
    env = {"KGE_RESCAL_FUSED": "1", "KGE_RESCAL_STAGED": "1"}
    tr, before, batch, after, pa, pb, sa, sb = _run_case(hip, monkeypatch, "rescal/neg1", "rescal", hp, E, R, B, world, env, "generic",
                                                         deterministic=False)
    assert getattr(tr, "_rescal_stage", None) is not None
    pairs_per_rel = np.bincount(batch[1], minlength=R)
    assert pairs_per_rel.max() > 64
    assert tr.rescal_reproducible is False
    norm = ko.rescal_normalize_tables(before, np.float64)
    grad = {n: norm[n] - after[n].astype(np.float64) for n in before}
    _check(hip, "rescal/neg1", "rescal", world[1], before, after, batch, hp, E, R, B, flat_grad=grad)


def test_rescal_with_several_negatives_is_refused_loudly(hip, monkeypatch):
    """The pairwise hinge adds [B] positives to [B * neg_rate] negatives (criterion.py:27), which only broadcasts at neg_rate 1: a
    RESCAL step with neg_rate 2 is refused, not run on some other grouping."""
    E, R, k, B = 3000, 7, 64, 256
    world = _world("rescal", E, R, B, dict(hidden_size=k), seed=2106)
    hp = dict(hidden_size=k, margin=1.0, neg_rate=2)
    tr, m = _trainer(hip, "rescal", hp, E, R, B, world, {"KGE_RESCAL_FUSED": "1", "KGE_RESCAL_STAGED": "1"}, monkeypatch)
    with pytest.raises(ValueError, match="neg_rate == 1"):
        tr.train_model_epoch(0)
