#!/usr/bin/env python
"""Dev tool: timed K.eval_ranks of TuckER and ProjE_pointwise (the shared rank pass of csrc/kge_projection.hip) at the reference
fixtures' shape (E = 70, d = 20, 12 queries: launch overheads) and at FB15k's shape with 512 queries.  Warm-up, then the median
[min, max] of 7 rounds of 5 back-to-back calls between two events.  KGE_HIP_LIB selects another build of the library for A/B runs.
Usage: python tools/projection_eval_perf.py >> profiles/r12_projection_scaffold.txt"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.projection import ProjE_pointwise, TuckER  # noqa: E402


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


rng = np.random.default_rng(3)
for E, R, D, n in ((70, 5, 20, 12), (14951, 1345, 200, 512)):
    trip = torch.from_numpy(np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1)).cuda()
    known = torch.from_numpy(np.stack([rng.integers(E, size=20 * n), rng.integers(R, size=20 * n), rng.integers(E, size=20 * n)], 1)).cuda()
    csr = K.filter_csr_build(torch.cat([known, trip]), trip, E, R)
    models = {"tucker": TuckER(tot_entity=E, tot_relation=R, ent_hidden_size=D, rel_hidden_size=D, lmbda=0.0, input_dropout=0.3,
                               hidden_dropout1=0.4, hidden_dropout2=0.5).cuda().eval(),
              "proje": ProjE_pointwise(tot_entity=E, tot_relation=R, hidden_size=D, lmbda=1e-5, hidden_dropout=0.5).cuda()}
    for name, m in models.items():
        d = m.make_desc()
        t = bench(lambda: K.eval_ranks(d, trip, *csr))
        print("eval_ranks %-6s E = %5d d = %3d n = %3d: %9.1f [%.1f, %.1f] us" % (name, E, D, n, *t))
