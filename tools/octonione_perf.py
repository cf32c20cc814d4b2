#!/usr/bin/env python
"""Step and eval timings of OctonionE on the HIP path against the same step in stock ATen ops on the same GPU.

The ATen side restates the reference's step (pykg2vec/models/pointwise.py:905-1001: 24 embedding gathers, _onorm, _omult from
_qmult / _qstar, the bilinear sum; Criterion.pointwise_logistic plus get_reg's N3 term; autograd; torch.optim.Adagrad over dense
tables) -- what the reference's Trainer runs per step.  Shapes: the FB15k-237 preset (hyperparams/OctonionE.yaml: d = 50, B = 100,
Adagrad lr 0.1, lmbda 0.2, neg_rate 1) and the same at B = 32 768.  The eval pass ranks 1 000 test triples.
Timing as in bench.py: CUDA events around a region of `--steps` steps, median over `--repeats` regions, after warm-up.

Usage:  python tools/octonione_perf.py [--steps 20] [--repeats 7] [--json out.json]
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

PRESET = dict(E=14541, R=237, hp=dict(hidden_size=50, lmbda=0.2, neg_rate=1), B=100, lr=0.1)
N_EVAL = 1000   # test triples per eval pass


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


def run(steps, repeats, B=None):
    import hip_util
    from test_octonione_model import energy64, reg64
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    E, R, hp, lr = PRESET["E"], PRESET["R"], PRESET["hp"], PRESET["lr"]
    B = B or PRESET["B"]
    rng = np.random.default_rng(0)
    trip = np.stack([rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)], 1)
    rows = np.repeat(trip, 2, 0)
    rows[1::2, 2] = rng.integers(E, size=B)
    y = np.tile(np.array([1, -1], np.int64), B)
    batch = [hip_util.dev(x) for x in (rows[:, 0], rows[:, 1], rows[:, 2], y)]
    m = hip_util.model_from_params("octonione", {}, hp, E, R)
    test = trip[:N_EVAL]
    tr = Trainer(m, hip_util.make_config(E, R, hp, trip, test, test, optimizer="adagrad", lr=lr, batch_size=B))
    tr.build_model()

    def hip_step():
        tr.train_step_pointwise(*batch)
        tr._reduce_and_step()
    res = {"model": "octonione", "E": E, "R": R, "B": B, "hp": hp}
    res["hip_step_ms"] = timed(hip_step, steps, repeats)
    desc = m.make_desc()
    tq = hip_util.dev(test)
    ws = K.eval_workspace(desc, len(test), tq.device)
    res["hip_eval_ms"] = timed(lambda: K.eval_ranks(desc, tq, None, None, None, None, workspace=ws), 1, repeats, warmup=1)

    # the ATen step over copies of the same tables (energy64 / reg64 are dtype-agnostic restatements of the reference's forward)
    P = {e.name: torch.nn.Parameter(e.weight.detach().clone()) for e in m.parameter_list[:16]}
    opt = torch.optim.Adagrad(list(P.values()), lr=lr)
    yf = batch[3].float()

    def aten_step():
        opt.zero_grad()
        loss = F.softplus(yf * energy64(P, *batch[:3])).mean() + hp["lmbda"] * reg64(P, *batch[:3], 3)
        loss.backward()
        opt.step()
    res["aten_step_ms"] = timed(aten_step, steps, repeats)
    ents = torch.arange(E, device=tq.device)

    def aten_eval():   # the reference's Evaluator: forward over all E candidates per test triple and side (utils/evaluator.py:254-272)
        with torch.no_grad():
            for lo in range(0, len(test), 16):
                q = tq[lo:lo + 16]
                n = q.shape[0]
                hh, rr, tt = (q[:, i:i + 1].expand(n, E).reshape(-1) for i in range(3))
                cand = ents.repeat(n)
                torch.argsort(energy64(P, hh, rr, cand).view(n, E), dim=1)
                torch.argsort(energy64(P, cand, rr, tt).view(n, E), dim=1)
    res["aten_eval_ms"] = timed(aten_eval, 1, 3, warmup=1)
    res["step_speedup"] = res["aten_step_ms"] / res["hip_step_ms"]
    res["eval_speedup"] = res["aten_eval_ms"] / res["hip_eval_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", default="preset,32768")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "octonione_perf.py needs a GPU"
    out = []
    for b in a.batches.split(","):
        r = run(a.steps, a.repeats, None if b == "preset" else int(b))
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
