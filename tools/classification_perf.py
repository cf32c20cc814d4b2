#!/usr/bin/env python
"""Dev tool: triple classification (csrc/kge_classify.hip, kge_corrupt_typed) at FB15k's shape: E = 14 951, R = 1 345, 59 071 positives
+ 59 071 negatives per split, relation ids uniform and Zipf(1.0).  Scores are given (random, continuous): scoring is not timed.
  (a) HIP       what Evaluator.fit_thresholds + test_classification launch: the per-relation fit and the global fit on the validation
                scores, classification_apply with labels and the AUC fit on the test scores
  (b) composed  the same four results from torch ops on the same GPU: a stable torch.sort of the combined key, cumsum, searchsorted for
                the segment and tie-group starts, a per-relation scatter_reduce(amax) of the packed cut word, scatter_add for the counts
(a) and (b) are checked to give the same thresholds, fit rows and confusion counts before they are timed.
  (c) kernels.corrupt_typed against kernels.corrupt (neg_rate 1) over 59 071 positives, set of 592 213 known triples
Warm-up, then the median [min, max] of 7 rounds of back-to-back calls between two events.
Usage: python tools/classification_perf.py > profiles/r08_classification.md"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.evaluator import build_type_constraints  # noqa: E402

E, R, N, N_TRAIN = 14951, 1345, 59071, 483142
NAN_KEY = 0xFFFFFFFF
BIAS = 1 << 30


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


def keys_torch(scores, higher):
    bits = scores.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
    asc = torch.where((bits & 0x80000000) != 0, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    key = (~asc & 0xFFFFFFFF) if higher else asc
    return torch.where(torch.isnan(scores), torch.full_like(key, NAN_KEY), key)


def composed_fit(scores, rel, label, n_rel, higher):
    n = scores.numel()
    comb = (rel << 33) | (keys_torch(scores, higher) << 1) | (1 - label.to(torch.int64))
    srt, _ = torch.sort(comb, stable=True)
    r, grp, pos = srt >> 33, srt >> 1, 1 - (srt & 1)
    k = grp & 0xFFFFFFFF
    idx = torch.arange(n, dtype=torch.int64, device=scores.device)
    cpos = torch.cumsum(pos, 0)
    before = cpos - pos                                   # positives in front of each position
    seg = torch.searchsorted(r, r)                        # first position of the relation
    first = torch.searchsorted(grp, grp)                  # first position of the tie group
    seg_pos = cpos - before[seg]
    value = 2 * seg_pos - (idx - seg + 1)
    last = torch.ones(n, dtype=torch.bool, device=scores.device)
    last[:-1] = grp[1:] != grp[:-1]
    word = torch.where(last & (k != NAN_KEY), ((value + BIAS) << 32) | (0xFFFFFFFF - (idx + 1)), torch.zeros_like(value))
    best = torch.full((n_rel,), (BIAS << 32) | 0xFFFFFFFF, dtype=torch.int64, device=scores.device).scatter_reduce(0, r, word, "amax")
    at = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    thr = torch.where(at > 0, k[(at - 1).clamp_(min=0)], torch.full_like(at, -1))
    neg = pos == 0
    rows = torch.zeros((n_rel, 6), dtype=torch.int64, device=scores.device)
    rows[:, 0].scatter_add_(0, r, pos)
    rows[:, 1].scatter_add_(0, r, 1 - pos)
    rows[:, 3].scatter_add_(0, r, torch.where(neg, before[first] - before[seg], torch.zeros_like(pos)))
    rows[:, 4].scatter_add_(0, r, torch.where(neg, cpos - before[first], torch.zeros_like(pos)))
    rows[:, 2] = (best >> 32) - BIAS + rows[:, 1]
    return thr, rows


def composed_apply(scores, rel, label, thr, seen, thr_global, higher):
    key = keys_torch(scores, higher)
    t = torch.where(seen[rel] != 0, thr[rel], torch.full_like(rel, thr_global))
    pred = (key != NAN_KEY) & (key <= t)
    lab = label != 0
    cell = torch.where(lab, torch.where(pred, 0, 3), torch.where(pred, 1, 2))
    conf = torch.zeros(thr.numel() * 4, dtype=torch.int64, device=scores.device)
    conf.scatter_add_(0, rel * 4 + cell, torch.ones_like(rel))
    return pred.to(torch.uint8), conf.view(-1, 4)


def relation_ids(rng, n, zipf):
    if not zipf:
        return rng.integers(0, R, size=n)
    p = 1.0 / np.arange(1, R + 1)
    return rng.choice(R, size=n, p=p / p.sum())


def fmt(t):
    return "%.3f ms [%.3f, %.3f]" % t


def main():
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    print("# Triple classification at the FB15k shape (E = %d, R = %d, 2 x %d labelled triples per split)\n" % (E, R, N))
    print("Device: %s.  Median [min, max] of 7 rounds of 3 back-to-back calls after 2 warm-up calls; scores are inputs.\n" % torch.cuda.get_device_name(0))
    print("| relation ids | HIP: 3 fits + apply | composed torch: 3 fits + apply | one HIP fit | one composed fit | HIP apply | composed apply |")
    print("|---|---|---|---|---|---|---|")
    for zipf in (False, True):
        split = []
        for _ in range(2):
            rel = np.tile(relation_ids(rng, N, zipf), 2)
            label = np.concatenate([np.ones(N, np.uint8), np.zeros(N, np.uint8)])
            scores = (rng.normal(size=2 * N) + 1.5 * (1 - label)).astype(np.float32)      # negatives score higher (an energy)
            split.append((torch.from_numpy(scores).to(dev), torch.from_numpy(rel).to(dev), torch.from_numpy(label).to(dev)))
        (vs, vr, vl), (ts, tr, tl) = split
        zeros = torch.zeros_like(vr)

        def hip():
            thr, fit = K.classification_fit(vs, vr, vl, R)
            gthr, _ = K.classification_fit(vs, zeros, vl, 1)
            seen = ((fit[:, 0] + fit[:, 1]) > 0).to(torch.uint8)
            return thr, fit, K.classification_apply(ts, tr, thr, seen, -1, label=tl)[1], K.classification_fit(ts, tr, tl, R)[1], gthr

        def composed():
            thr, fit = composed_fit(vs, vr, vl, R, False)
            gthr, _ = composed_fit(vs, zeros, vl, 1, False)
            seen = ((fit[:, 0] + fit[:, 1]) > 0).to(torch.uint8)
            return thr, fit, composed_apply(ts, tr, tl, thr, seen, -1, False)[1], composed_fit(ts, tr, tl, R, False)[1], gthr

        for a, b in zip(hip(), composed()):
            assert torch.equal(a, b), "the composed form disagrees with the HIP path"
        thr, fit = K.classification_fit(vs, vr, vl, R)
        seen = ((fit[:, 0] + fit[:, 1]) > 0).to(torch.uint8)
        print("| %s | %s | %s | %s | %s | %s | %s |" % (
            "Zipf(1.0)" if zipf else "uniform", fmt(bench(hip)), fmt(bench(composed)),
            fmt(bench(lambda: K.classification_fit(vs, vr, vl, R))), fmt(bench(lambda: composed_fit(vs, vr, vl, R, False))),
            fmt(bench(lambda: K.classification_apply(ts, tr, thr, seen, -1, label=tl))),
            fmt(bench(lambda: composed_apply(ts, tr, tl, thr, seen, -1, False)))))
    # ---- negatives
    train = np.stack([rng.integers(E, size=N_TRAIN), relation_ids(rng, N_TRAIN, True), rng.integers(E, size=N_TRAIN)], 1).astype(np.int64)
    pos = train[rng.integers(N_TRAIN, size=N)]
    extra = np.stack([rng.integers(E, size=N_TRAIN // 4), relation_ids(rng, N_TRAIN // 4, True), rng.integers(E, size=N_TRAIN // 4)], 1)
    known = torch.from_numpy(np.concatenate([train, extra]).astype(np.int64)).to(dev)
    slots = K.triple_set_build(known)
    ranges, domains = build_type_constraints(train, R)
    off = torch.stack([domains.off, ranges.off + domains.ids.numel()]).contiguous().to(dev)
    ids = torch.cat([domains.ids, ranges.ids]).contiguous().to(dev)
    ph, pr, pt = (torch.from_numpy(np.ascontiguousarray(pos[:, i])).to(dev) for i in range(3))
    neg, failed = K.corrupt_typed(ph, pr, pt, E, R, None, off, ids, slots, 1, 0)
    print("\n| negatives for %d positives (%d known triples, Zipf relations) | time | rows without a negative |" % (N, known.shape[0]))
    print("|---|---|---|")
    print("| kernels.corrupt_typed | %s | %d |" % (fmt(bench(lambda: K.corrupt_typed(ph, pr, pt, E, R, None, off, ids, slots, 1, 0))), int(failed.item())))
    print("| kernels.corrupt (uniform, neg_rate 1) | %s | - |" % fmt(bench(lambda: K.corrupt(ph, pr, pt, 1, E, None, slots, 1, 0))))


if __name__ == "__main__":
    main()
