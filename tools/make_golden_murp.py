#!/usr/bin/env python
"""Freeze the LIVE reference's MuRP outputs into tests/golden/ref_murp{,_k40,_ties}.npz (build container only: the reference tree is
imported through oracle/ref_shim.py).  Fixed seeds: a second run writes identical arrays.

  ref_murp       E = 97, R = 7, k = 10, neg_rate 3, 8 bundles.  The init state under the seed; tables in the live regime (0.12 * randn)
                 with three entity rows and one relation row pushed outside the ball and random bs / bo; a batch with id 0 as head, tail
                 and relation, one entity repeated in many rows and at least one saturated row; preds, loss, the five gradients; the
                 tables after one RiemannianOptimizer.step(lr = 50) and after one SGD step; a 4-step riemannian trajectory on recorded
                 batches from the init state; for 40 queries both predict_*_rank lists and the reference MetricCalculator's raw and
                 filtered ranks under a known-triple filter.
  ref_murp_k40   k = 40 (the yaml's width), neg_rate 50, 4 bundles: the step quantities only.
  ref_murp_ties  bs = bo = 0 and a third of the entity rows outside the ball: rank lists and ranks, for the tie band.

Branch margins.  Every norm the forward compares with 1 and every clamp argument is asserted to sit at least 1e-10 (relative) away from
its bounds, in float64 (tools/murp_reference.py recomputes them), so float64 and long double take the same branches: the reductions
here are 10 to 40 terms long, so two float64 evaluations differ by some 1e-15, five orders below the margin.  (A wider margin cannot
be had with these fixtures: a row clipped into the ball lands 1e-5 / |x| outside norm 1 by construction, p_sum of such a row lands
within 1e-6 of it, and a riemannian step at lr = 50 saturates tanh and leaves the row some 1e-9 inside norm 1.)  For ref_murp no
candidate's score may equal the true one's bit for bit and neighbouring scores of a sweep must be 1e-9 apart.  Otherwise the next seed
is tried; the seed used is written into the file.

The reference's MetricCalculator walks a candidate list from its END (utils/evaluator.py: tail_candidate[-j - 1]), and MuRP's lists are
ascending in the score: its ranks count the candidates that score HIGHER than the true one (rank_order = 1 of kge_murp_desc); the
position in the list itself is the rank_order = 0 count.  Both are recorded.

Usage:  python tools/make_golden_murp.py [ref_murp|ref_murp_k40|ref_murp_ties ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
import torch  # noqa: E402
from pykg2vec.models.pointwise import MuRP  # noqa: E402
from pykg2vec.utils.criterion import Criterion  # noqa: E402
from pykg2vec.utils.riemannian_optimizer import RiemannianOptimizer  # noqa: E402
from pykg2vec.utils.evaluator import MetricCalculator  # noqa: E402
from tools import murp_reference as mr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAMES = ("wu", "bs", "bo", "ent_embeddings.weight", "rel_embeddings.weight")
MARGIN = 1e-10
SCORE_GAP = 1e-9


class Retry(Exception):
    pass


def build(E, R, k, seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    return MuRP(tot_entity=E, tot_relation=R, hidden_size=k, lmbda=0.0, device="cpu")


def state(model):
    sd = model.state_dict()
    assert tuple(sd.keys()) == NAMES, tuple(sd.keys())
    return [sd[n].detach().numpy().copy() for n in NAMES]


def set_state(model, tabs):
    with torch.no_grad():
        for (name, p), a in zip(model.named_parameters(), tabs):
            p.copy_(torch.from_numpy(np.asarray(a)))


def live_tables(rng, E, R, k, outside_ent, outside_rel, zero_bias=False):
    ent = 0.12 * rng.standard_normal((E, k))
    rel = 0.12 * rng.standard_normal((R, k))
    for e in outside_ent:
        ent[e] *= rng.uniform(1.2, 2.5) / np.linalg.norm(ent[e])
    for r in outside_rel:
        rel[r] *= rng.uniform(1.2, 2.0) / np.linalg.norm(rel[r])
    wu = rng.uniform(-1, 1, (R, k))
    bs = np.zeros(E) if zero_bias else 0.3 * rng.standard_normal(E)
    bo = np.zeros(E) if zero_bias else 0.3 * rng.standard_normal(E)
    return [wu, bs, bo, ent, rel]


def make_batch(rng, E, R, n_pos, neg_rate, hub=None, force=()):
    """Bundles [positive, its neg_rate negatives]; `force`: positives written over the first bundles; hub: an entity many rows share."""
    h, r, t, y = [], [], [], []
    for i in range(n_pos):
        ph, pr, pt = (int(rng.integers(E)), int(rng.integers(R)), int(rng.integers(E))) if i >= len(force) else force[i]
        if hub is not None and i % 2 == 1:
            ph = hub
        h.append(ph); r.append(pr); t.append(pt); y.append(1)
        for j in range(neg_rate):
            if rng.random() < 0.5:
                h.append(int(rng.integers(E)) if hub is None or j % 3 else hub); t.append(pt)
            else:
                h.append(ph); t.append(int(rng.integers(E)) if hub is None or j % 3 else hub)
            r.append(pr); y.append(-1)
    return tuple(np.asarray(a, np.int64) for a in (h, r, t, y))


def check_margins(tabs, h, r, t, what):
    """No norm near 1, no clamp argument near its bounds (float64)."""
    _, s = mr.forward(tabs, h, r, t, np.float64, keep=True)
    hi = 1 - 1e-5
    for key in ("nh", "nt", "nr", "num", "nvm"):                       # compared with 1 by the clips
        if np.any(np.abs(s[key] - 1) < MARGIN):
            raise Retry("%s: %s within %g of 1" % (what, key, MARGIN))
    for key in ("nh1", "nz"):                                          # clamp(., 1e-10, 1 - 1e-5)
        v = s[key]
        if np.any(np.abs(v - hi) < MARGIN * hi) or np.any(np.abs(v - 1e-10) < MARGIN * 1e-10):
            raise Retry("%s: %s near a clamp bound" % (what, key))
    if np.any(np.abs(s["nwr"] - 1e-10) < MARGIN * 1e-10):
        raise Retry("%s: |u_w| near its clamp bound" % what)
    for ps in (s["ps1"], s["ps2"]):                                     # clamp(., 0, 1 - 1e-5) inside p_sum
        for v in ps[:2]:
            if np.any(np.abs(v - hi) < MARGIN * hi):
                raise Retry("%s: a p_sum squared norm near its clamp bound" % what)
    return s


def step_record(model, tabs, batch, lr, prefix, rec):
    """preds, loss, gradients, and the tables after one riemannian / one SGD step from `tabs`."""
    h, r, t, y = batch
    set_state(model, tabs)
    model.zero_grad()
    H, R_, T, Y = (torch.from_numpy(a) for a in (h, r, t, y))
    preds = model.forward(H, R_, T)
    loss = Criterion.pointwise_bce(preds, Y.double())
    loss.backward()
    grads = [p.grad.detach().numpy().copy() for _, p in model.named_parameters()]
    rec[prefix + "preds"] = preds.detach().numpy().copy()
    rec[prefix + "loss"] = np.float64(loss.item())
    for n, g in zip(NAMES, grads):
        rec[prefix + "grad." + n] = g
    params = [p for _, p in model.named_parameters()]
    opt = RiemannianOptimizer(params, lr=lr, param_names=[n for n, _ in model.named_parameters()])
    opt.step()
    for n, a in zip(NAMES, state(model)):
        rec[prefix + "riemannian." + n] = a
    set_state(model, tabs)
    with torch.no_grad():
        for p, g in zip(params, grads):
            p.sub_(lr * torch.from_numpy(g))
    for n, a in zip(NAMES, state(model)):
        rec[prefix + "sgd." + n] = a
    return grads


def trajectory(model, init, batches, lr, rec):
    set_state(model, init)
    params = [p for _, p in model.named_parameters()]
    opt = RiemannianOptimizer(params, lr=lr, param_names=[n for n, _ in model.named_parameters()])
    losses = []
    for i, (h, r, t, y) in enumerate(batches):
        check_margins(state(model), h, r, t, "trajectory step %d" % i)
        model.zero_grad()
        loss = Criterion.pointwise_bce(model.forward(*(torch.from_numpy(a) for a in (h, r, t))), torch.from_numpy(y).double())
        loss.backward()
        opt.step()
        losses.append(loss.item())
        for k_, a in zip(("h", "r", "t", "y"), (h, r, t, y)):
            rec["traj.batch%d.%s" % (i, k_)] = a
    rec["traj.loss"] = np.asarray(losses, np.float64)
    for n, a in zip(NAMES, state(model)):
        rec["traj.after." + n] = a


def rank_record(model, tabs, rng, E, R, n_q, rec, want_no_ties):
    set_state(model, tabs)
    known = np.stack([rng.integers(E, size=400), rng.integers(R, size=400), rng.integers(E, size=400)], 1).astype(np.int64)
    queries = known[rng.choice(len(known), n_q, replace=False)].copy()
    queries[0] = (0, 0, 0)
    known = np.concatenate([known, queries[:1]])
    hr_t, tr_h = {}, {}
    for h, r, t in known:
        hr_t.setdefault((int(h), int(r)), set()).add(int(t))
        tr_h.setdefault((int(t), int(r)), set()).add(int(h))
    mc = MetricCalculator.__new__(MetricCalculator)
    mc.hr_t, mc.tr_h = hr_t, tr_h
    ents = np.arange(E)
    tails, heads, out = [], [], {k_: [] for k_ in ("rank_head", "rank_tail", "frank_head", "frank_tail", "pos_head", "pos_tail")}
    model.eval()
    with torch.no_grad():
        for h, r, t in queries:
            h, r, t = int(h), int(r), int(t)
            check_margins(tabs, np.full(E, h), np.full(E, r), ents, "tail sweep")
            check_margins(tabs, ents, np.full(E, r), np.full(E, t), "head sweep")
            tl = model.predict_tail_rank(torch.LongTensor([h]), torch.LongTensor([r]), topk=-1).numpy()
            hl = model.predict_head_rank(torch.LongTensor([t]), torch.LongTensor([r]), topk=-1).numpy()
            for lst, row, true in ((tl, model.forward(torch.full((E,), h), torch.full((E,), r), torch.arange(E)).numpy(), t),
                                   (hl, model.forward(torch.arange(E), torch.full((E,), r), torch.full((E,), t)).numpy(), h)):
                if want_no_ties:
                    srt = np.sort(row)
                    if np.any(np.diff(srt) < SCORE_GAP * np.maximum(1.0, np.abs(srt[1:]))):
                        raise Retry("two candidates of a sweep score within %g" % SCORE_GAP)
            tr_, ftr = mc.get_tail_rank(tl, h, r, t)
            hr_, fhr = mc.get_head_rank(hl, h, r, t)
            tails.append(tl); heads.append(hl)
            out["rank_tail"].append(tr_); out["frank_tail"].append(ftr); out["rank_head"].append(hr_); out["frank_head"].append(fhr)
            out["pos_tail"].append(int(np.flatnonzero(tl == t)[0])); out["pos_head"].append(int(np.flatnonzero(hl == h)[0]))
    rec["eval.known"] = known
    rec["eval.queries"] = queries
    rec["eval.tail_list"] = np.asarray(tails, np.int64)
    rec["eval.head_list"] = np.asarray(heads, np.int64)
    for k_, v in out.items():
        rec["eval." + k_] = np.asarray(v, np.int64)


def golden_main(seed):
    E, R, k, neg, n_pos, lr = 97, 7, 10, 3, 8, 50.0
    rng = np.random.default_rng(seed)
    model = build(E, R, k, seed)
    rec = {"seed": np.int64(seed), "E": np.int64(E), "R": np.int64(R), "k": np.int64(k), "neg_rate": np.int64(neg), "lr": np.float64(lr)}
    init = state(model)
    for n, a in zip(NAMES, init):
        rec["init." + n] = a
    outside_ent, outside_rel = (5, 23, 61), (3,)
    tabs = live_tables(rng, E, R, k, outside_ent, outside_rel)
    for n, a in zip(NAMES, tabs):
        rec["live." + n] = a
    batch = make_batch(rng, E, R, n_pos, neg, hub=11, force=[(0, 0, 0), (5, 3, 23), (61, 2, 40)])
    s = check_margins(tabs, *batch[:3], "batch")
    sat = s["nz"] > 1 - 1e-5
    if not sat.any() or sat.all():
        raise Retry("the batch needs saturated and live rows (%d of %d saturated)" % (sat.sum(), len(sat)))
    rec["batch.saturated"] = sat
    for k_, a in zip(("h", "r", "t", "y"), batch):
        rec["batch." + k_] = a
    grads = step_record(model, tabs, batch, lr, "step.", rec)
    if not all(np.abs(g).max() > 0 for g in grads):
        raise Retry("a gradient is all zero")
    traj_tabs = [a.copy() for a in init]
    trajectory(model, traj_tabs, [make_batch(rng, E, R, n_pos, neg, hub=11) for _ in range(4)], lr, rec)
    rank_record(model, tabs, rng, E, R, 40, rec, want_no_ties=True)
    return "ref_murp", rec


def golden_k40(seed):
    E, R, k, neg, n_pos, lr = 97, 7, 40, 50, 4, 50.0
    rng = np.random.default_rng(seed)
    model = build(E, R, k, seed)
    rec = {"seed": np.int64(seed), "E": np.int64(E), "R": np.int64(R), "k": np.int64(k), "neg_rate": np.int64(neg), "lr": np.float64(lr)}
    tabs = live_tables(rng, E, R, k, (9, 70), (5,))
    for n, a in zip(NAMES, tabs):
        rec["live." + n] = a
    batch = make_batch(rng, E, R, n_pos, neg, hub=11, force=[(0, 0, 0)])
    check_margins(tabs, *batch[:3], "batch")
    for k_, a in zip(("h", "r", "t", "y"), batch):
        rec["batch." + k_] = a
    step_record(model, tabs, batch, lr, "step.", rec)
    return "ref_murp_k40", rec


def golden_ties(seed):
    E, R, k = 97, 7, 10
    rng = np.random.default_rng(seed)
    model = build(E, R, k, seed)
    rec = {"seed": np.int64(seed), "E": np.int64(E), "R": np.int64(R), "k": np.int64(k)}
    tabs = live_tables(rng, E, R, k, tuple(range(1, E, 3)), (), zero_bias=True)
    for n, a in zip(NAMES, tabs):
        rec["live." + n] = a
    rank_record(model, tabs, rng, E, R, 40, rec, want_no_ties=False)
    return "ref_murp_ties", rec


CASES = {"ref_murp": (golden_main, 7101), "ref_murp_k40": (golden_k40, 7201), "ref_murp_ties": (golden_ties, 7301)}

if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (fn, seed0) in CASES.items():
        if only and name not in only:
            continue
        for seed in range(seed0, seed0 + 50):
            try:
                name, rec = fn(seed)
                break
            except Retry as e:
                print("%s: seed %d refused (%s)" % (name, seed, e))
        else:
            raise SystemExit("%s: no seed passed the margins" % name)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **rec)
        print("wrote %s (seed %d, %d bytes)" % (path, seed, os.path.getsize(path)))
