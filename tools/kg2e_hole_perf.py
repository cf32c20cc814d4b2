#!/usr/bin/env python
"""Step and eval timings of KG2E / HoLE on the HIP path against the same step in stock ATen ops on the same GPU.

The ATen side restates the reference's forward (pykg2vec/models/pairwise.py:1035-1142: row norms, the KL sums; for HoLE
torch.fft with the torch < 1.7 semantics, i.e. real and imaginary parts multiplied elementwise), Criterion.pairwise_hinge,
autograd and torch.optim.SGD over dense tables -- what the reference's Trainer runs per step.  Shapes: the FB15k presets
(hyperparams/KG2E.yaml, HoLE.yaml) and the same at B = 32 768.
Timing as in bench.py: CUDA events around a region of `--steps` steps, median over `--repeats` regions, after warm-up.

Usage:  python tools/kg2e_hole_perf.py [--steps 20] [--repeats 7] [--json out.json]
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

PRESETS = {   # FB15k: KG2E hidden 50, batch 1440; HoLE hidden 150, batch 1200; both SGD
    "kg2e": dict(E=14951, R=1345, hp=dict(hidden_size=50, cmax=0.05, cmin=5.0, margin=4.0), B=1440, lr=0.01),
    "hole": dict(E=14951, R=1345, hp=dict(hidden_size=150, cmax=0.05, cmin=5.0, margin=0.2), B=1200, lr=0.1),
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
    if model == "kg2e":
        nz = lambda x: x.div(torch.norm(x, 2, 1).view(-1, 1).expand_as(x))
        hm, hs, rm, rs = nz(P["ent_mu"][h]), nz(P["ent_sigma"][h]), nz(P["rel_mu"][r]), nz(P["rel_sigma"][r])
        tm, ts = nz(P["ent_mu"][t]), nz(P["ent_sigma"][t])
        cs, cm = hs + rs, hm + rm
        return (cs / ts).sum(-1) + ((tm - cm) ** 2 / ts).sum(-1) + (torch.log(ts) - torch.log(cs)).sum(-1) - hm.shape[1]
    eh, et = P["ent"][h], P["ent"][t]
    rr = F.normalize(P["rel"][r], p=2, dim=-1)
    fh, ft = torch.fft.fft(eh), torch.fft.fft(et)
    # legacy semantics: conj is the identity on the real-pair tensor and `*` multiplies re*re and im*im
    prod = torch.complex(fh.real * ft.real, fh.imag * ft.imag)
    e = torch.fft.ifft(prod).real
    return -torch.sigmoid(torch.sum(rr * e, 1))


def run(model, steps, repeats, B=None):
    import hip_util
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    p = PRESETS[model]
    E, R, hp = p["E"], p["R"], p["hp"]
    B = B or p["B"]
    rng = np.random.default_rng(0)
    trip = np.stack([rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)], 1)
    neg = trip.copy()
    neg[:, 2] = rng.integers(E, size=B)
    batch = [hip_util.dev(x) for x in (trip[:, 0], trip[:, 1], trip[:, 2], neg[:, 0], neg[:, 1], neg[:, 2])]
    m = hip_util.model_from_params(model, {}, hp, E, R)
    test = trip[:N_EVAL]
    tr = Trainer(m, hip_util.make_config(E, R, hp, trip, test, test, optimizer="sgd", lr=p["lr"], batch_size=B))
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
    names = ["ent_mu", "ent_sigma", "rel_mu", "rel_sigma"] if model == "kg2e" else ["ent", "rel"]
    P = {n: torch.nn.Parameter(e.weight.detach().clone()) for n, e in zip(names, m.parameter_list)}
    opt = torch.optim.SGD(list(P.values()), lr=p["lr"])

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
    ap.add_argument("--models", default="kg2e,hole")
    ap.add_argument("--batches", default="preset,32768")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kg2e_hole_perf.py needs a GPU"
    out = []
    for model in a.models.split(","):
        for b in a.batches.split(","):
            r = run(model, a.steps, a.repeats, None if b == "preset" else int(b))
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
