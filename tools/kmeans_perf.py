#!/usr/bin/env python
"""Dev tool: k-means (csrc/kge_kmeans.hip) at FB15k's shape (E = 14 951, d = 100, float32 normal rows), k = 16, 100, 1000: the time
per Lloyd iteration of K.kmeans_run and the time of K.kmeans_seed, against the torch composition a user wrote before -- matmul plus the
norm terms into an [n, k] block, argmin, index_add_ (float atomics) and a division.  The baseline is not the code under test.  Warm-up,
then the median [min, max] of 7 rounds of 40 back-to-back calls between two events, the rounds of the two paths alternating.  A
fused call includes a copy of the start centroids and its output allocations.
Usage: python tools/kmeans_perf.py > profiles/r32_kmeans_perf.txt
       python tools/kmeans_perf.py --trace     (a few iterations and one seeding per k: for a kernel trace)"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402

ITERS = 20


def bench(fns, warm=2, rounds=7, inner=40):
    """One (median, min, max) in us per call for every function: the rounds of the functions alternate, so that a drift of the
    machine falls on all of them; a round is `inner` back-to-back calls between two events (0.1 s and more at these shapes)."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for fn, times in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / inner * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in out]


def composed(X, C, iters):
    """Lloyd's iteration from torch ops: an [n, k] key block per iteration, centroid sums through index_add_."""
    xn = (X * X).sum(1)
    for _ in range(iters):
        label = ((C * C).sum(1)[None, :] - 2 * torch.matmul(X, C.t())).argmin(1)
        sums = torch.zeros_like(C).index_add_(0, label, X)
        count = torch.zeros(C.shape[0], device=X.device).index_add_(0, label, torch.ones_like(xn))
        C = torch.where(count[:, None] > 0, sums / count.clamp(min=1)[:, None], C)
    return C, label


def fused(X, C0, iters):
    return K.kmeans_run(X, C0.clone(), iters)


E, D = 14951, 100
rng = np.random.default_rng(11)
X = torch.from_numpy(rng.normal(size=(E, D)).astype(np.float32)).cuda()
trace = "--trace" in sys.argv
if not trace:
    print("command: python tools/kmeans_perf.py   (E = %d, d = %d, float32 normal rows, %d Lloyd iterations per call; %s)"
          % (E, D, ITERS, torch.cuda.get_device_name(0)))
for k in (16, 100, 1000):
    u = torch.from_numpy(rng.random(k)).cuda()
    C0 = X[torch.from_numpy(rng.permutation(E)[:k]).cuda()].contiguous()
    if trace:
        fused(X, C0, 3)
        K.kmeans_seed(X, k, u)
        continue
    # both paths run the same number of iterations: those the fused run needs before it stops (all ITERS unless it converges)
    iters = int(fused(X, C0, ITERS).state[1].item())
    (t_run, t_base), (t_seed,) = bench([lambda: fused(X, C0, iters), lambda: composed(X, C0, iters)]), bench([lambda: K.kmeans_seed(X, k, u)], inner=5)
    same = float((fused(X, C0, iters).label.long() == composed(X, C0, iters)[1]).float().mean())
    ratio = t_base[0] / t_run[0]
    print("k = %4d, %2d iterations: kmeans_run %8.1f [%.1f, %.1f] us per iteration   torch composition %8.1f [%.1f, %.1f] us per iteration   "
          "ratio %.2f (%s; %.2f%% of the labels agree)   kmeans_seed %9.1f [%.1f, %.1f] us (%.1f us per centre)"
          % (k, iters, *(t / iters for t in t_run), *(t / iters for t in t_base), ratio, "fused FASTER" if ratio > 1 else "fused SLOWER",
             100 * same, *t_seed, t_seed[0] / k))
torch.cuda.synchronize()
