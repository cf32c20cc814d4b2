#!/usr/bin/env python
"""Dev tool: ranking against given candidates (csrc/kge_candidates.hip) at FB15k's shape (E = 14 951, TransE L1, d = 100) and WN18's
(E = 40 943, ComplEx, d = 200): 4096 queries, both sides, C candidates per query and side, with and without filter lists (20 known
entities per query and side).  Three paths for the same job:
  (a) fused     K.rank_candidates, twice (tails, heads)
  (b) composed  what the library offered before: the [n, C] lists expanded to n * C explicit triples, K.score_forward over them and
                over the true triples, the four counts in torch (the filter as a sorted-key membership test)
  (c) sweep     K.eval_ranks over all E entities for the same queries (what Evaluator.rank_all runs); independent of C
(a) and (b) are checked to give the same counts before they are timed.  Warm-up, then the median [min, max] of 7 rounds of
back-to-back calls between two events.
Usage: python tools/candidates_perf.py > profiles/r22_candidates_perf.txt"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pykg2vec_amd as pa  # noqa: E402
from pykg2vec_amd import kernels as K  # noqa: E402


def bench(fn, warm=2, rounds=7, inner=3):
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
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out), min(out), max(out)


def composed_side(desc, q, side, table, E, skip):
    """int32 [4, n] through explicit triples: what a caller had to write before kge_rank_candidates."""
    n, C = table.shape
    col = 0 if side else 2
    cand = table.reshape(-1)
    h = cand if side else q[:, 0].repeat_interleave(C)
    r = q[:, 1].repeat_interleave(C)
    t = q[:, 2].repeat_interleave(C) if side else cand
    live = ((table >= 0) & (table < E) & (table != q[:, col:col + 1]))
    safe = torch.where(live.reshape(-1), cand, torch.zeros_like(cand))          # dead entries score a placeholder row
    s = K.score_forward(desc, safe if side else h.contiguous(), r.contiguous(), t.contiguous() if side else safe).view(n, C)
    s_true = K.score_forward(desc, q[:, 0].contiguous(), q[:, 1].contiguous(), q[:, 2].contiguous()).view(n, 1)
    kept = live
    if skip is not None:
        off, ids = skip
        pos = torch.arange(ids.numel(), dtype=torch.int64, device=ids.device)
        keys = (torch.searchsorted(off, pos, right=True) - 1) * E + ids.to(torch.int64)      # ascending: the segments are sorted
        want = torch.arange(n, dtype=torch.int64, device=ids.device).view(n, 1) * E + table
        at = torch.searchsorted(keys, want.reshape(-1)).clamp_(max=keys.numel() - 1)
        kept = live & (keys[at] != want.reshape(-1)).view(n, C)
    lt, eq = s < s_true, s == s_true
    return torch.stack([(lt & live).sum(1), (lt & kept).sum(1), (eq & live).sum(1), (eq & kept).sum(1)]).to(torch.int32)


def run(tag, model, E, R, d, hp, n=4096, known=20):
    rng = np.random.default_rng(22)
    m = pa.import_model(model)(tot_entity=E, tot_relation=R, hidden_size=d, **hp).cuda()
    desc = m.make_desc()
    q = torch.from_numpy(np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1).astype(np.int64)).cuda()
    skips = []
    for side in (0, 1):
        ids = np.sort(rng.integers(E, size=(n, known)), axis=1).astype(np.int32)
        skips.append((torch.arange(n + 1, dtype=torch.int64, device="cuda") * known, torch.from_numpy(ids.reshape(-1)).cuda()))
    sweep = bench(lambda: K.eval_ranks(desc, q, skips[0][0], skips[0][1], skips[1][0], skips[1][1]))
    print("%s: %s d = %d, E = %d, %d queries, both sides; (c) full sweep K.eval_ranks %9.3f [%.3f, %.3f] ms" % (tag, model, d, E, n, *sweep))
    print("%-6s %-8s %28s %28s %9s %9s" % ("C", "filter", "(a) fused ms", "(b) composed ms", "(b)/(a)", "(c)/(a)"))
    for C in (64, 500, 1000, 4096):
        tables = [torch.from_numpy(rng.integers(E, size=(n, C)).astype(np.int64)).cuda() for _ in (0, 1)]
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * C
        ids32 = [t.reshape(-1).to(torch.int32) for t in tables]
        for filt in (False, True):
            sk = lambda side: skips[side] if filt else (None, None)
            fused = lambda: [K.rank_candidates(desc, q, side, off, ids32[side], skip_off=sk(side)[0], skip_ids=sk(side)[1], skip_sorted=True)
                             for side in (0, 1)]
            composed = lambda: [composed_side(desc, q, side, tables[side], E, skips[side] if filt else None) for side in (0, 1)]
            for x, y in zip(fused(), composed()):
                assert torch.equal(x, y), "fused and composed counts differ"
            a, b = bench(fused), bench(composed)
            print("%-6d %-8s %9.3f [%8.3f, %8.3f] %9.3f [%8.3f, %8.3f] %9.2f %9.2f"
                  % (C, "yes" if filt else "no", *a, *b, b[0] / a[0], sweep[0] / a[0]))
            del fused, composed
        del tables, ids32
        torch.cuda.empty_cache()


print("command: python tools/candidates_perf.py   (%s; KGE_CAND_CHUNK = %d)" % (torch.cuda.get_device_name(0), K.CAND_CHUNK))
run("FB15k", "transe", 14951, 1345, 100, dict(l1_flag=True, margin=1.0))
run("WN18", "complex", 40943, 18, 200, dict(lmbda=0.01))
