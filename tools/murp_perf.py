#!/usr/bin/env python
"""Step and rank timings of MuRP on the HIP path against the same work in stock ATen float64 ops on the same GPU.

The ATen side restates what the reference's Trainer runs per step from the formulas of DESIGN.md section 24 (gathers, clips, the two
maps, p_sum, the distance; BCE-with-logits; autograd; the Riemannian update of the two embeddings and p -= lr g on wu, bs, bo) and
its Evaluator's forward over all candidates with the sort behind it.  Shape: FB15k (E = 14 951, R = 1 345), k = 40, neg_rate 50,
lr 50, B = 128 (hyperparams/MuRP.yaml) and B = 4 096; a step scores B * 51 rows.  Timing: CUDA events around a region of `--steps`
steps, median over `--repeats` regions, after warm-up; nothing else runs in the process.

Usage:  python tools/murp_perf.py [--steps 10] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPE = dict(E=14951, R=1345, hp=dict(hidden_size=40, neg_rate=50, lmbda=0.0), lr=50.0)
N_EVAL = 200   # test triples per rank pass


def timed(fn, steps, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out)


def _norm(x):
    return torch.norm(x, 2, dim=-1, keepdim=True)


def _clip(x):
    n = _norm(x)
    return torch.where(n >= 1, x / (n - 1e-5), x)


def _arsech(x):
    return torch.log((1 + torch.sqrt(1 - x * x)) / x)


def _p_sum(x, y):
    sx = torch.clamp((x * x).sum(-1, keepdim=True), 0, 1 - 1e-5)
    sy = torch.clamp((y * y).sum(-1, keepdim=True), 0, 1 - 1e-5)
    d = (x * y).sum(-1, keepdim=True)
    return ((1 + 2 * d + sy) * x + (1 - sx) * y) / (1 + 2 * d + sx * sy)


def aten_forward(P, h, r, t):
    wu, bs, bo, ent, rel = P
    hc, tc, rc = _clip(ent[h]), _clip(ent[t]), _clip(rel[r])
    c = torch.clamp(_norm(hc), 1e-10, 1 - 1e-5)
    uw = (_arsech(c) * hc / c) * wu[r]
    nw = torch.clamp(_norm(uw), min=1e-10)
    um = _clip((1 / torch.cosh(nw)) * uw / nw)
    vm = _clip(_p_sum(tc, rc))
    dist = 2 * _arsech(torch.clamp(torch.norm(_p_sum(-um, vm), 2, dim=-1), 1e-10, 1 - 1e-5))
    return -(dist * dist - bs[h] - bo[t])


def aten_rsgd(P, lr):
    with torch.no_grad():
        for p in P[:3]:
            p -= lr * p.grad
        for p in P[3:]:
            sq = torch.clamp((p * p).sum(-1, keepdim=True), 0, 1 - 1e-5)
            v = -lr * (p.grad * ((1 - sq) ** 2 / 4))
            nv = torch.clamp(_norm(v), min=1e-10)
            p.copy_(_p_sum(p, torch.tanh(nv / (1 - sq)) * v / nv))


def run(steps, repeats, B):
    import hip_util
    import pykg2vec_amd as pa
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    E, R, hp, lr = SHAPE["E"], SHAPE["R"], SHAPE["hp"], SHAPE["lr"]
    neg = hp["neg_rate"]
    rng = np.random.default_rng(0)
    n_trip = max(B, N_EVAL)
    trip = np.stack([rng.integers(E, size=n_trip), rng.integers(R, size=n_trip), rng.integers(E, size=n_trip)], 1)
    rows = np.repeat(trip[:B], 1 + neg, 0)
    corrupt = np.ones(len(rows), bool)
    corrupt[::1 + neg] = False
    rows[corrupt, 2] = rng.integers(E, size=int(corrupt.sum()))
    y = np.where(corrupt, -1, 1).astype(np.int64)
    batch = [hip_util.dev(x) for x in (rows[:, 0], rows[:, 1], rows[:, 2], y)]
    test = trip[:N_EVAL]
    res = {"model": "murp", "E": E, "R": R, "B": B, "rows_per_step": len(rows), "hp": hp, "optimizer": "riemannian", "lr": lr}

    torch.manual_seed(0)
    np.random.seed(0)
    m = pa.import_model("murp")(tot_entity=E, tot_relation=R, device="cuda", **{k: v for k, v in hp.items() if k != "neg_rate"}).to("cuda")
    with torch.no_grad():   # the live regime: the shipped 1e-3 init saturates nothing and moves little
        m.ent_embeddings.weight.copy_(0.06 * torch.randn_like(m.ent_embeddings.weight))
        m.rel_embeddings.weight.copy_(0.06 * torch.randn_like(m.rel_embeddings.weight))
    start = [p.detach().clone() for p in m.trainable_tensors()]
    tr = Trainer(m, hip_util.make_config(E, R, hp, trip, test, test, optimizer="riemannian", lr=lr, batch_size=B))
    tr.build_model()

    def hip_step():
        tr.train_step_pointwise(*batch)
        tr._reduce_and_step()
    res["hip_step_ms"] = timed(hip_step, steps, repeats)
    with torch.no_grad():
        for p, s in zip(m.trainable_tensors(), start):
            p.copy_(s)
    desc = m.make_desc()
    tq = hip_util.dev(test)
    res["hip_rank_ms"] = timed(lambda: K.eval_ranks(desc, tq, None, None, None, None), 1, repeats, warmup=1)

    P = [torch.nn.Parameter(s.clone()) for s in start]
    yf = torch.clamp(batch[3].double(), 0, 1)

    def aten_step():
        for p in P:
            p.grad = None
        F.binary_cross_entropy_with_logits(aten_forward(P, *batch[:3]), yf).backward()
        aten_rsgd(P, lr)
    res["aten_step_ms"] = timed(aten_step, steps, repeats)
    ents = torch.arange(E, device=tq.device)

    def aten_rank():   # the reference's Evaluator: forward over all E candidates per test triple and side, then the sort
        with torch.no_grad():
            for i in range(len(test)):
                h, r, t = (tq[i, j].expand(E) for j in range(3))
                torch.sort(aten_forward(P, h, r, ents))
                torch.sort(aten_forward(P, ents, r, t))
    res["aten_rank_ms"] = timed(aten_rank, 1, 3, warmup=1)
    res["eval_triples"] = len(test)
    res["step_speedup"] = res["aten_step_ms"] / res["hip_step_ms"]
    res["rank_speedup"] = res["aten_rank_ms"] / res["hip_rank_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "murp_perf.py needs a GPU"
    out = []
    for b in a.batches.split(","):
        r = run(a.steps, a.repeats, int(b))
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
