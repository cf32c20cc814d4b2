#!/usr/bin/env python
"""Dev tool: relation ranking (csrc/kge_relations.hip) at FB15k's shape -- E = 14 951, R = 1 345, n = 8 192 queries on seeded uniform
ids, three known relations per pair as skip segments -- for TransE-L1 d = 100, ComplEx d = 200 and RotatE d = 1000.  Paths for the
same job:
  (a) fused        K.rank_relations
  (b) composed     what the library offered before, from entry points of the parent commit only: the R - 1 other relations of every
                   query expanded to explicit triples, K.score_forward over them and over the true triples, K.rank_lists_from_scores
                   with "kept" flags; the expansion (index arithmetic in torch) is part of the call
  (b') composed, ids ready   the same with the expanded id tensors and flags built once outside the timed window: score + count only
(a) and (b) are checked to give the same counts before they are timed.  The paths are alternated inside one process: warm-up of every
path, then 7 rounds, each timing every path between two events with a device synchronise; median [min, max] per call.
Usage: python tools/relation_rank_perf.py > profiles/r07_relation_rank.md"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pykg2vec_amd as pa  # noqa: E402
from pykg2vec_amd import kernels as K  # noqa: E402

ROUNDS, WARM = 7, 2


def alternate(paths, inner):
    """{name: (median, min, max) ms per call}; every round times each path once, in turn."""
    for fn in paths.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner[k]):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / inner[k])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def expand(q, R, skip_off, skip_ids):
    """(h, r, t, flags, seg) of the R - 1 other relations of every query, true triples in front."""
    n = q.shape[0]
    dev = q.device
    others = torch.arange(R - 1, dtype=torch.int64, device=dev).unsqueeze(0)
    rel = others + (others >= q[:, 1:2]).to(torch.int64)
    known = torch.zeros((n, R), dtype=torch.bool, device=dev)
    row = torch.searchsorted(skip_off, torch.arange(skip_ids.numel(), dtype=torch.int64, device=dev), right=True) - 1
    known[row, skip_ids.to(torch.int64)] = True
    flags = (((~known.gather(1, rel)).reshape(-1).to(torch.uint8) << 1) | 1).contiguous()
    h = torch.cat([q[:, 0], q[:, 0].repeat_interleave(R - 1)]).contiguous()
    r = torch.cat([q[:, 1], rel.reshape(-1)]).contiguous()
    t = torch.cat([q[:, 2], q[:, 2].repeat_interleave(R - 1)]).contiguous()
    seg = torch.arange(n + 1, dtype=torch.int64, device=dev) * (R - 1)
    return h, r, t, flags, seg


def score_and_count(desc, n, h, r, t, flags, seg):
    s = K.score_forward(desc, h, r, t)
    return K.rank_lists_from_scores(s[n:], s[:n].contiguous(), seg, flags)


def run(model, d, hp, E=14951, R=1345, n=8192, known=3):
    rng = np.random.default_rng(7)
    m = pa.import_model(model)(tot_entity=E, tot_relation=R, hidden_size=d, **hp).cuda()
    desc = m.make_desc()
    qn = np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1).astype(np.int64)
    lists = [sorted({int(r)} | set(rng.integers(R, size=known - 1).tolist())) for r in qn[:, 1]]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)).cuda()
    ids = torch.from_numpy(np.asarray([e for x in lists for e in x], dtype=np.int32)).cuda()
    q = torch.from_numpy(qn).cuda()
    ready = expand(q, R, off, ids)
    paths = {"fused": lambda: K.rank_relations(desc, q, off, ids, skip_sorted=True),
             "composed": lambda: score_and_count(desc, n, *expand(q, R, off, ids)),
             "composed, ids ready": lambda: score_and_count(desc, n, *ready)}
    want = paths["fused"]()
    assert torch.equal(want, paths["composed"]()) and torch.equal(want, paths["composed, ids ready"]()), "fused and composed counts differ"
    assert int((want[1] < want[0]).sum()) > 0
    res = alternate(paths, {"fused": 5, "composed": 2, "composed, ids ready": 2})
    f = res["fused"][0]
    for k, (med, lo, hi) in res.items():
        print("| %s d = %d | %s | %.3f | %.3f | %.3f | %.2f |" % (model, d, k, med, lo, hi, med / f))


print("# Relation ranking: fused kernel against the composed path")
print()
print("command: `python tools/relation_rank_perf.py` on %s; KGE_REL_CHUNK = %d; E = 14 951, R = 1 345, n = 8 192 seeded uniform queries, "
      "three known relations per pair; paths alternated in one process, %d warm-up calls each, %d rounds, event timing with a device "
      "synchronise per window." % (torch.cuda.get_device_name(0), K.REL_CHUNK, WARM, ROUNDS))
print()
print("| model | path | median ms per call | min | max | median / fused |")
print("|---|---|---|---|---|---|")
run("transe", 100, dict(l1_flag=True, margin=1.0))
run("complex", 200, dict(lmbda=0.01))
run("rotate", 1000, dict(margin=6.0))
