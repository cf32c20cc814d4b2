#!/usr/bin/env python
"""Step and rank timings of ConvKB on the HIP path against the same work in stock ATen ops on the same GPU.

The ATen side restates the reference's step (pykg2vec/models/pointwise.py:302-318: three gathers, the stacked [b, 1, 3, k] input,
one conv2d per filter width, cat, fc1; Criterion.pointwise_logistic; autograd; torch.optim.Adam over the two dense tables and fc1)
-- what the reference's Trainer runs per step -- and its Evaluator's forward over all candidates.  Shape: FB15k (E = 14 951,
R = 1 345), k = 100, F = 50, widths [1, 2], neg_rate 1, B = 128 (hyperparams/ConvKB.yaml) and B = 4 096.  DistMult's HIP step at the
same shape is reported for scale.  Timing: CUDA events around a region of `--steps` steps, median over `--repeats` regions, after
warm-up; nothing else runs in the process.

Usage:  python tools/convkb_perf.py [--steps 20] [--repeats 5] [--json out.json]
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

SHAPE = dict(E=14951, R=1345, hp=dict(hidden_size=100, num_filters=50, filter_sizes=[1, 2], neg_rate=1), lr=0.01)
N_EVAL = 1000   # test triples per rank pass


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


def run(steps, repeats, B):
    import hip_util
    import pykg2vec_amd as pa
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.trainer import Trainer
    E, R, hp, lr = SHAPE["E"], SHAPE["R"], SHAPE["hp"], SHAPE["lr"]
    rng = np.random.default_rng(0)
    trip = np.stack([rng.integers(E, size=max(B, N_EVAL)), rng.integers(R, size=max(B, N_EVAL)), rng.integers(E, size=max(B, N_EVAL))], 1)
    rows = np.repeat(trip[:B], 2, 0)
    rows[1::2, 2] = rng.integers(E, size=B)
    y = np.tile(np.array([1, -1], np.int64), B)
    batch = [hip_util.dev(x) for x in (rows[:, 0], rows[:, 1], rows[:, 2], y)]
    test = trip[:N_EVAL]
    res = {"model": "convkb", "E": E, "R": R, "B": B, "hp": hp, "optimizer": "adam"}

    def hip_step_of(model, hp_):
        tr = Trainer(model, hip_util.make_config(E, R, hp_, trip, test, test, optimizer="adam", lr=lr, batch_size=B))
        tr.build_model()

        def step():
            tr.train_step_pointwise(*batch)
            tr._reduce_and_step()
        return step

    torch.manual_seed(0)
    m = pa.import_model("convkb")(tot_entity=E, tot_relation=R, device="cuda", **{k: v for k, v in hp.items() if k != "neg_rate"}).to("cuda")
    res["hip_step_ms"] = timed(hip_step_of(m, hp), steps, repeats)
    dm = hip_util.model_from_params("distmult", {}, dict(hidden_size=hp["hidden_size"], lmbda=0.0), E, R)
    res["distmult_hip_step_ms"] = timed(hip_step_of(dm, dict(hidden_size=hp["hidden_size"], lmbda=0.0, neg_rate=1)), steps, repeats)
    desc = m.make_desc()
    tq = hip_util.dev(test)
    res["hip_rank_ms"] = timed(lambda: K.eval_ranks(desc, tq, None, None, None, None), 1, repeats, warmup=1)

    # the ATen step over copies of the same tensors
    ent, rel = (torch.nn.Parameter(p.detach().clone()) for p in (m.ent_embeddings.weight, m.rel_embeddings.weight))
    fc_w, fc_b = (torch.nn.Parameter(p.detach().clone()) for p in (m.fc1.weight, m.fc1.bias))
    convs = [(c.weight.detach().to("cuda"), c.bias.detach().to("cuda")) for c in m.conv_list]
    opt = torch.optim.Adam([ent, rel, fc_w, fc_b], lr=lr)
    yf = batch[3].float()

    def forward(h, r, t):
        x = torch.stack([ent[h], rel[r], ent[t]], 1).unsqueeze(1)
        z = torch.cat([F.conv2d(x, w, b) for w, b in convs], 3)
        return F.linear(z.view(h.numel(), -1), fc_w, fc_b).squeeze(-1)

    def aten_step():
        opt.zero_grad()
        F.softplus(yf * forward(*batch[:3])).mean().backward()
        opt.step()
    res["aten_step_ms"] = timed(aten_step, steps, repeats)
    ents = torch.arange(E, device=tq.device)

    def aten_rank():   # the reference's Evaluator: forward over all E candidates per test triple and side (utils/evaluator.py:254-272)
        with torch.no_grad():
            for lo in range(0, len(test), 4):
                q = tq[lo:lo + 4]
                n = q.shape[0]
                hh, rr, tt = (q[:, i:i + 1].expand(n, E).reshape(-1) for i in range(3))
                cand = ents.repeat(n)
                torch.argsort(forward(hh, rr, cand).view(n, E), dim=1)
                torch.argsort(forward(cand, rr, tt).view(n, E), dim=1)
    res["aten_rank_ms"] = timed(aten_rank, 1, 3, warmup=1)
    res["step_speedup"] = res["aten_step_ms"] / res["hip_step_ms"]
    res["rank_speedup"] = res["aten_rank_ms"] / res["hip_rank_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "convkb_perf.py needs a GPU"
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
