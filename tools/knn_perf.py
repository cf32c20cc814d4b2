#!/usr/bin/env python
"""Dev tool: the nearest-neighbour search (csrc/kge_knn.hip) at FB15k's shape (E = 14 951, d = 100, float32): K.knn_rows for 1 024
queries and for all 14 951, k = 10 and 100, the three metrics, against the composition the library offered before it --
torch.matmul (plus the norm terms) into a score block of at most 1 024 rows, then K.topk_rows on the block.  The baseline is not the
code under test.  Warm-up, then the median [min, max] of 7 rounds of back-to-back calls between two events.
Usage: python tools/knn_perf.py > profiles/r26_knn_perf.txt
       python tools/knn_perf.py --trace     (the fused calls of the 1 024-query shapes only, a few times: for a kernel trace)"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402


def bench(fn, warm=3, rounds=7, inner=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner * 1e3)
    return statistics.median(out), min(out), max(out)


def composed(table, queries, k, metric, chunk=1024):
    """What a user wrote before knn_rows: a [chunk, E] score block per chunk of queries, then the row select."""
    tn2 = (table * table).sum(1) if metric != "dot" else None
    ids, vals = [], []
    for a in range(0, queries.shape[0], chunk):
        q = queries[a:a + chunk]
        s = torch.matmul(q, table.t())
        if metric == "cosine":
            s = s / ((q * q).sum(1).sqrt()[:, None] * tn2.sqrt()[None, :])
        elif metric == "l2":
            s = ((q * q).sum(1)[:, None] + tn2[None, :] - 2 * s).clamp_(min=0)
        i, v, _ = K.topk_rows(s, k, largest=metric != "l2")
        ids.append(i)
        vals.append(v)
    return torch.cat(ids), torch.cat(vals)


E, D = 14951, 100
rng = np.random.default_rng(11)
table = torch.from_numpy(rng.normal(size=(E, D)).astype(np.float32)).cuda()
if "--trace" in sys.argv:
    for metric in ("dot", "cosine", "l2"):
        for _ in range(5):
            K.knn_rows(table, table[:1024], 10, metric=metric)
    torch.cuda.synchronize()
    sys.exit(0)

print("command: python tools/knn_perf.py   (E = %d, d = %d, float32 normal rows; the queries are the first table rows; %s)"
      % (E, D, torch.cuda.get_device_name(0)))
for nq in (1024, E):
    queries = table[:nq]
    for k in (10, 100):
        for metric in ("dot", "cosine", "l2"):
            rounds = dict(rounds=7, inner=5 if nq == 1024 else 1)
            fused = bench(lambda: K.knn_rows(table, queries, k, metric=metric), **rounds)
            base = bench(lambda: composed(table, queries, k, metric), **rounds)
            same = float((K.knn_rows(table, queries, k, metric=metric)[0] == composed(table, queries, k, metric)[0]).all(1).float().mean())
            ratio = base[0] / fused[0]
            note = "fused FASTER than matmul + topk_rows" if ratio > 1 else "fused SLOWER than matmul + topk_rows"
            print("%5d queries k = %3d %-6s: knn_rows %9.1f [%.1f, %.1f] us   matmul + topk_rows %9.1f [%.1f, %.1f] us   ratio %.2f  (%s; "
                  "%.1f%% of the rows list the same ids)" % (nq, k, metric, *fused, *base, ratio, note, 100 * same))
