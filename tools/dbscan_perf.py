#!/usr/bin/env python
"""Dev tool: DBSCAN (csrc/kge_dbscan.hip) at FB15k's shape (E = 14 951, d = 100, float32 rows: 64 unit Gaussian blobs around N(0, 1)
centres), eps from Evaluator.suggest_eps at min_samples = 5 and 20: the fused call K.dbscan against the torch composition a user wrote
before -- one torch.cdist block [n, n] and its threshold, counts by row sum, the core-by-core boolean block, components by repeated
masked min over it until stable, then the border rows.  The baseline is not the code under test.  Warm-up, then the median [min, max]
of 7 rounds of 3 back-to-back calls between two events, the rounds of the two paths alternating.  A fused call includes its workspace
and output allocations and its one host read per labelling round.  Peak device memory: the fused call's workspace
(kge_dbscan_workspace_bytes) and outputs against torch's peak allocation during the composition.  The card is shared: times move from
run to run; the ratio of alternating rounds is the steadier figure.
Usage: python tools/dbscan_perf.py > profiles/r34_dbscan_perf.txt"""
import os
import statistics
import sys
import types

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K, _lib as L  # noqa: E402
from pykg2vec_amd.evaluator import Evaluator  # noqa: E402


def bench(fns, warm=2, rounds=7, inner=3):
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


def composed(X, eps, min_samples):
    """DBSCAN from torch ops: the [n, n] block, then min-id propagation over the boolean core block until nothing moves."""
    n = X.shape[0]
    near = torch.cdist(X, X) <= eps
    near.fill_diagonal_(True)
    count = near.sum(1)
    core = count >= min_samples
    ids = torch.nonzero(core).flatten()
    m = int(ids.numel())
    graph = near[ids][:, ids]
    comp = torch.arange(m, device=X.device)
    big = torch.full((1,), m, device=X.device)
    sweeps = 0
    while True:
        sweeps += 1
        new = torch.where(graph, comp[None, :], big).min(1).values
        new = new[new]                                             # one pointer jump
        if torch.equal(new, comp):
            break
        comp = new
    number = torch.cumsum((comp == torch.arange(m, device=X.device)).long(), 0) - 1
    label = torch.full((n,), -1, dtype=torch.int64, device=X.device)
    reach = torch.where(near[:, ids], number[comp][None, :], big).min(1).values if m else label
    label = torch.where(reach < m, reach, label) if m else label
    return label, count, sweeps


E, D = 14951, 100
rng = np.random.default_rng(11)
centres = rng.normal(size=(64, D))
X = torch.from_numpy((centres[rng.integers(0, 64, E)] + rng.normal(size=(E, D))).astype(np.float32)).cuda()
ev = Evaluator.__new__(Evaluator)
ev.K, ev.model = K, types.SimpleNamespace(entity_matrix=lambda tables: X)
print("command: python tools/dbscan_perf.py   (E = %d, d = %d, 64 Gaussian blobs; %s; a shared card)" % (E, D, torch.cuda.get_device_name(0)))
for min_samples in (5, 20):
    eps = ev.suggest_eps(min_samples)
    t_fused, t_base = bench([lambda: K.dbscan(X, eps, min_samples), lambda: composed(X, eps, min_samples)])
    res, again = K.dbscan(X, eps, min_samples), K.dbscan(X, eps, min_samples)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    label, count, sweeps = composed(X, eps, min_samples)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    ws = L.load().kge_dbscan_workspace_bytes(E, D)
    ratio = t_base[0] / t_fused[0]
    print("min_samples = %2d, eps = %.4f: dbscan %9.1f [%.1f, %.1f] us, %d labelling rounds   torch composition %9.1f [%.1f, %.1f] us, %d sweeps   "
          "ratio %.2f (%s)   clusters %d, cores %d, noise %d   labels differ on %d rows, counts on %d (float32 pairs at eps may), "
          "results repeat: %s   device memory: fused %.2f MB (workspace %.2f MB), composition peak %.1f MB"
          % (min_samples, eps, *t_fused, int(res.rounds.item()), *t_base, sweeps, ratio, "fused FASTER" if ratio > 1 else "fused SLOWER",
             int(res.n_clusters.item()), int(res.core.sum()), int((res.label < 0).sum()), int((res.label.long() != label).sum()),
             int((res.count.long() != count).sum()), all(torch.equal(getattr(res, f), getattr(again, f)) for f in res._fields),
             (ws + 9 * E + 8) / 1e6, ws / 1e6, peak / 1e6))
torch.cuda.synchronize()
