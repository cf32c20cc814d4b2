#!/usr/bin/env python
"""Dev tool: the silhouette (csrc/kge_silhouette.hip) at FB15k's shape (E = 14 951, d = 100, float32 normal rows, labels = the nearest of
k random rows), k = 16, 100, 1000: the fused call K.silhouette against two torch compositions a user wrote before -- torch.cdist in row
blocks of 2048 rows into a [2048, n] block, the per-cluster sums of a block either by a float64 index_add_ (float atomics, which
collide where k is small) or by a float64 GEMM with the one-hot label matrix (no atomics), then the means, the minimum and the
score.  The baselines are not the code under test.  Warm-up, then the median [min, max] of 7 rounds of 10 back-to-back calls between
two events, the rounds of the three paths alternating.  A fused call includes its workspace and output
allocations.  Peak device memory: the fused call's workspace (kge_silhouette_workspace_bytes) and outputs, against the composition's
[2048, n] float32 block, its float64 copy and the [n, k] float64 sums (the one-hot form adds the [n, k] float64 label matrix).
Usage: python tools/silhouette_perf.py > profiles/r33_silhouette_perf.txt
       python tools/silhouette_perf.py --trace K   (three fused calls at k = K and nothing else: the program of a kernel trace,
                                                    rocprofv3 --kernel-trace --stats --output-format csv, one run per k)"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K, _lib as L  # noqa: E402

BLOCK = 2048


def bench(fns, warm=2, rounds=7, inner=10):
    """One (median, min, max) in us per call for every function: the rounds of the functions alternate, so that a drift of the
    machine falls on all of them; a round is `inner` back-to-back calls between two events."""
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


def composed(X, label, k, gemm=False):
    """The silhouette from torch ops: row blocks of the distance matrix, per-cluster sums in float64 through index_add_, or
    (gemm) through a product with the one-hot label matrix."""
    n = X.shape[0]
    count = torch.bincount(label, minlength=k).double()
    sums = torch.empty((n, k), dtype=torch.float64, device=X.device)
    own = torch.nn.functional.one_hot(label, k).bool()
    hot = own.double() if gemm else None
    for r0 in range(0, n, BLOCK):
        D = torch.cdist(X[r0:r0 + BLOCK], X).double()             # [BLOCK, n]: d(i, i) is 0 up to rounding and adds nothing
        sums[r0:r0 + BLOCK] = D @ hot if gemm else torch.zeros((D.shape[0], k), dtype=torch.float64, device=X.device).index_add_(1, label, D)
    a = sums[own] / (count[label] - 1).clamp(min=1)
    b = torch.where(own | (count[None, :] == 0), torch.full_like(sums, float("inf")), sums / count.clamp(min=1)[None, :]).min(1).values
    s = torch.where(count[label] > 1, (b - a) / torch.maximum(a, b), torch.zeros_like(a))
    return s.float(), s.float().double().mean()


E, D = 14951, 100
rng = np.random.default_rng(11)
X = torch.from_numpy(rng.normal(size=(E, D)).astype(np.float32)).cuda()
trace = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else None
if not trace:
    print("command: python tools/silhouette_perf.py   (E = %d, d = %d, float32 normal rows; %s)" % (E, D, torch.cuda.get_device_name(0)))
for k in (trace,) if trace else (16, 100, 1000):
    C = X[torch.from_numpy(rng.permutation(E)[:k]).cuda()]
    label = torch.cdist(X, C).argmin(1)
    label32 = label.to(torch.int32)
    if trace:
        for _ in range(3):
            K.silhouette(X, label32, k)
        continue
    t_fused, t_base, t_gemm = bench([lambda: K.silhouette(X, label32, k), lambda: composed(X, label, k), lambda: composed(X, label, k, gemm=True)])
    res, (s_base, score_base) = K.silhouette(X, label32, k), composed(X, label, k)
    again = K.silhouette(X, label32, k)
    ratio, ratio_gemm = t_base[0] / t_fused[0], t_gemm[0] / t_fused[0]
    ws = L.load().kge_silhouette_workspace_bytes(E, D, k)
    print("k = %4d: silhouette %9.1f [%.1f, %.1f] us   torch composition: index_add_ %9.1f [%.1f, %.1f] us   ratio %.2f (%s); one-hot GEMM %9.1f [%.1f, %.1f] us   ratio %.2f (%s)   %.1f TFLOP/s of 2 n^2 d   "
          "max |s - composition| %.2e, score %.6f vs %.6f, bits repeat: %s   device memory: fused %.2f MB (workspace %.2f MB), "
          "composition %.1f MB"
          % (k, *t_fused, *t_base, ratio, "fused FASTER" if ratio > 1 else "fused SLOWER", *t_gemm, ratio_gemm,
             "fused FASTER" if ratio_gemm > 1 else "fused SLOWER", 2.0 * E * E * D / t_fused[0] / 1e6,
             float((res.s - s_base).abs().max()), res.score.item(), score_base.item(),
             all(torch.equal(getattr(res, f).view(torch.uint8), getattr(again, f).view(torch.uint8)) for f in res._fields),
             (ws + 4 * (4 * E + k) + 8) / 1e6, ws / 1e6, (BLOCK * E * 12 + 2 * E * k * 8) / 1e6))   # (one-hot form: + E k 8 bytes)
torch.cuda.synchronize()
