#!/usr/bin/env python
"""Dev tool: the row select (csrc/kge_topk.hip) and the batched link prediction at FB15k's shape (E = 14 951, TransE d = 100,
1024 queries), k = 10 and k = 1000.
  - K.topk_rows against torch.topk on the same [1024, E] float32 rows: random normals (the common case), rows quantised to 8 levels
    (LDS histogram atomics collide), and the masked form with 20 known ids per row.
  - Evaluator.predict_tails over 1024 (h, r) pairs in one call against 1024 calls of Evaluator.test_tail_rank, both ending in a
    device synchronise (host clock: the per-query path is bound by its host round trips).
Warm-up, then the median [min, max] of 7 rounds of back-to-back calls between two events.
Usage: python tools/topk_perf.py > profiles/r21_topk_perf.txt"""
import os
import statistics
import sys
import time
import types

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pykg2vec_amd as pa  # noqa: E402
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.evaluator import Evaluator  # noqa: E402


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


def wall(fn, warm=1, rounds=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


E, R, D, NQ = 14951, 1345, 100, 1024
rng = np.random.default_rng(11)
print("command: python tools/topk_perf.py   (E = %d, R = %d, d = %d, %d queries; %s)" % (E, R, D, NQ, torch.cuda.get_device_name(0)))

rows = {"normal": torch.from_numpy(rng.normal(size=(NQ, E)).astype(np.float32)).cuda(),
        "8 levels": torch.from_numpy((np.floor(rng.random((NQ, E)) * 8) / 4 - 1).astype(np.float32)).cuda()}
off = torch.arange(NQ + 1, dtype=torch.int64, device="cuda") * 20
ids = torch.from_numpy(rng.integers(E, size=20 * NQ).astype(np.int32)).cuda()
for k in (10, 1000):
    for name, x in rows.items():
        ours = bench(lambda: K.topk_rows(x, k))
        theirs = bench(lambda: torch.topk(x, k, largest=False))
        masked = bench(lambda: K.topk_rows(x, k, skip_off=off, skip_ids=ids))
        note = "select slower than torch.topk" if ours[0] > theirs[0] else "select faster than torch.topk"
        print("rows %-8s k = %4d: topk_rows %8.1f [%.1f, %.1f] us   torch.topk %8.1f [%.1f, %.1f] us   masked topk_rows %8.1f [%.1f, %.1f] us   (%s)"
              % (name, k, *ours, *theirs, *masked, note))

trip = np.stack([rng.integers(E, size=60000), rng.integers(R, size=60000), rng.integers(E, size=60000)], 1).astype(np.int64)
kg = types.SimpleNamespace(cache={"triplets_train": trip[:50000], "triplets_valid": trip[50000:55000], "triplets_test": trip[55000:]})
kg.read_cache_data = lambda key: kg.cache[key]
cfg = types.SimpleNamespace(tot_entity=E, tot_relation=R, device="cuda", knowledge_graph=kg, hits=[1, 3, 10], debug=False, test_num=0)
m = pa.import_model("transe")(tot_entity=E, tot_relation=R, hidden_size=D, l1_flag=True, margin=1.0).cuda()
ev = Evaluator(m, cfg)
q = trip[55000:55000 + NQ]
h, r = torch.from_numpy(q[:, 0]).cuda(), torch.from_numpy(q[:, 1]).cuda()
hl, rl = q[:, 0].tolist(), q[:, 1].tolist()
for k in (10, 1000):
    batched = wall(lambda: ev.predict_tails(h, r, topk=k))
    filtered = wall(lambda: ev.predict_tails(h, r, topk=k, filtered=True))
    single = wall(lambda: [ev.test_tail_rank(a, b, topk=k) for a, b in zip(hl, rl)], rounds=3)
    print("TransE tails of %d queries, k = %4d: predict_tails %8.2f [%.2f, %.2f] ms   filtered %8.2f [%.2f, %.2f] ms   %d x test_tail_rank %8.2f [%.2f, %.2f] ms"
          % (NQ, k, *batched, *filtered, NQ, *single))
