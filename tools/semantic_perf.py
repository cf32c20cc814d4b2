#!/usr/bin/env python
"""Step and eval timings of SLM / SME / SME_BL on the HIP path against the same step in stock ATen ops on the same GPU.

The ATen side restates the reference's forward (pykg2vec/models/pairwise.py:473-724: F.normalize, matmuls, tanh / sums),
Criterion.pairwise_hinge, autograd and torch.optim.Adam over dense tables -- what the reference's Trainer runs per step.
Timing as in bench.py: CUDA events around a region of `--steps` steps, median over `--repeats` regions, after warm-up.

Usage:  python tools/semantic_perf.py [--steps 20] [--repeats 7] [--json out.json]
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

PRESETS = {   # hyperparams/*.yaml of the reference: SME on FB15k (hidden 50, batch 50 000, Adam); SLM 64 / 32, batch 128
    "sme": dict(E=14951, R=1345, hp=dict(hidden_size=50, margin=1.0), B=50000),
    "sme_bl": dict(E=14951, R=1345, hp=dict(hidden_size=50, margin=1.0), B=50000),
    "slm": dict(E=14951, R=1345, hp=dict(ent_hidden_size=64, rel_hidden_size=32, margin=1.0), B=128),
}
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


def aten_energy(model, P, h, r, t):
    hn, rn, tn = (F.normalize(x, p=2, dim=-1) for x in (P["ent"][h], P["rel"][r], P["ent"][t]))
    if model == "slm":
        return -torch.sum(rn * torch.tanh(hn @ P["mr1"] + tn @ P["mr2"]), -1)
    a, b = torch.matmul(P["mu1"], hn.T), torch.matmul(P["mu2"], rn.T)
    c, d = torch.matmul(P["mv1"], tn.T), torch.matmul(P["mv2"], rn.T)
    if model == "sme":
        return -torch.sum((a + b + P["bu"]).T * (c + d + P["bv"]).T, 1)
    return torch.sum((a * b + P["bu"]).T * (c * d + P["bv"]).T, -1)


def run(model, steps, repeats):
    import hip_util
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    p = PRESETS[model]
    E, R, B, hp = p["E"], p["R"], p["B"], p["hp"]
    rng = np.random.default_rng(0)
    trip = np.stack([rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)], 1)
    neg = trip.copy()
    neg[:, 2] = rng.integers(E, size=B)
    batch = [hip_util.dev(x) for x in (trip[:, 0], trip[:, 1], trip[:, 2], neg[:, 0], neg[:, 1], neg[:, 2])]
    m = hip_util.model_from_params(model, {}, hp, E, R)
    test = trip[:N_EVAL]
    tr = Trainer(m, hip_util.make_config(E, R, hp, trip, test, test, optimizer="adam", lr=1e-3, batch_size=B))
    tr.build_model()

    def hip_step():
        tr.train_step_pairwise(*batch)
        tr._reduce_and_step()
    res = {"model": model, "E": E, "R": R, "B": B, "hp": hp}
    res["hip_step_ms"] = timed(hip_step, steps, repeats)
    desc = m.make_desc()
    tq = hip_util.dev(test)
    ws = K.eval_workspace(desc, N_EVAL, tq.device)
    res["hip_eval_ms"] = timed(lambda: K.eval_ranks(desc, tq, None, None, None, None, workspace=ws), 1, repeats, warmup=1)

    # the ATen step over copies of the same tables
    names = ["ent", "rel", "mr1", "mr2"] if model == "slm" else ["ent", "rel", "mu1", "mu2", "bu", "mv1", "mv2", "bv"]
    P = {n: torch.nn.Parameter(e.weight.detach().clone()) for n, e in zip(names, m.parameter_list)}
    opt = torch.optim.Adam(list(P.values()), lr=1e-3)

    def aten_step():
        opt.zero_grad()
        pos, ng = aten_energy(model, P, *batch[:3]), aten_energy(model, P, *batch[3:])
        torch.sum(F.relu(pos + hp["margin"] - ng)).backward()
        opt.step()
    res["aten_step_ms"] = timed(aten_step, steps, repeats)
    ents = torch.arange(E, device=tq.device)

    def aten_eval():   # the reference's Evaluator: forward over all E candidates per test triple and side (utils/evaluator.py:254-272)
        with torch.no_grad():
            for lo in range(0, N_EVAL, 16):
                q = tq[lo:lo + 16]
                n = q.shape[0]
                hh, rr, tt = (q[:, i:i + 1].expand(n, E).reshape(-1) for i in range(3))
                cand = ents.repeat(n)
                torch.argsort(aten_energy(model, P, hh, rr, cand).view(n, E), dim=1)
                torch.argsort(aten_energy(model, P, cand, rr, tt).view(n, E), dim=1)
    res["aten_eval_ms"] = timed(aten_eval, 1, 3, warmup=1)
    res["step_speedup"] = res["aten_step_ms"] / res["hip_step_ms"]
    res["eval_speedup"] = res["aten_eval_ms"] / res["hip_eval_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--models", default="sme,sme_bl,slm")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "semantic_perf.py needs a GPU"
    out = []
    for model in a.models.split(","):
        r = run(model, a.steps, a.repeats)
        print(json.dumps(r))
        out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
