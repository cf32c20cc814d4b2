#!/usr/bin/env python
"""Freeze the LIVE reference's ConvKB outputs into tests/golden/ref_convkb{,_neg3}.npz (build container only: oracle/make_golden.py
imports the reference tree through oracle/ref_shim.py).  The recipe is oracle/make_golden.py's golden_for, called unchanged.

golden_for rebuilds the model seven times, and the reference's ConvKB keeps its filters in a plain list: every rebuild would draw
fresh random filters that no state_dict carries.  make_golden.build is a module global, so it is wrapped here: the first build's
filters are recorded and copied into every later build, and written to the fixture afterwards as conv.{j}.weight / conv.{j}.bias.

Every recorded rank is then checked in float64 (the affine form of tools/convkb_reference.py on the eval.after.* weights): the true
candidate's nearest competitor must be farther than MIN_GAP away in each of the 24 sweeps -- about 20 times the fp32 disagreement
between the reference and the affine form -- and the float64 ranks must equal the recorded ones.  That is what entitles the GPU test
to demand exact ranks.  Fixed seeds: a second run writes identical arrays.

  convkb       hidden_size = 20, num_filters = 5, filter_sizes = [1, 3, 2] (not sorted: the column layout off_j is pinned), neg_rate 1
  convkb_neg3  the same with neg_rate = 3

Usage:  python tools/make_golden_convkb.py [convkb|convkb_neg3 ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import make_golden  # noqa: E402
import torch  # noqa: E402
from tools import convkb_reference as cr  # noqa: E402

CASES = {
    "convkb": ("pointwise.ConvKB", dict(hidden_size=20, num_filters=5, filter_sizes=[1, 3, 2]), 4401),
    "convkb_neg3": ("pointwise.ConvKB", dict(hidden_size=20, num_filters=5, filter_sizes=[1, 3, 2], neg_rate=3), 4402),
}
MIN_GAP = 1e-6


def golden_with_fixed_filters(name, cls_path, hp, seed):
    original = make_golden.build
    first = []

    def build(cls_path, cfg, init_state=None):
        model = original(cls_path, cfg, init_state)
        if not first:
            first.extend((c.weight.detach().clone(), c.bias.detach().clone()) for c in model.conv_list)
        with torch.no_grad():
            for c, (w, b) in zip(model.conv_list, first):
                c.weight.copy_(w)
                c.bias.copy_(b)
        return model

    make_golden.build = build
    try:
        make_golden.golden_for(name, cls_path, hp, seed)
    finally:
        make_golden.build = original
    path = os.path.join(make_golden.OUT, "ref_%s.npz" % name)
    rec = dict(np.load(path))
    for j, (w, b) in enumerate(first):
        rec["conv.%d.weight" % j] = w.numpy().copy()
        rec["conv.%d.bias" % j] = b.numpy().copy()
    check_rank_gaps(name, rec)
    np.savez_compressed(path, **rec)
    print("wrote", name, "with", len(first), "filters;", os.path.getsize(path), "bytes")


def check_rank_gaps(name, rec):
    P = cr.params_from_fixture(rec, "eval.after.")
    E = int(rec["E"])
    n = len(rec["eval.rank_head"])
    allt = np.concatenate([rec["train"], rec["valid"], rec["test"]])
    gaps = {"head": [], "tail": []}
    for i, (h, r, t) in enumerate(rec["test"][:n]):
        ents = np.arange(E)
        for side, row, true in (("tail", cr.preds64(P, np.full(E, h), np.full(E, r), ents), int(t)),
                                ("head", cr.preds64(P, ents, np.full(E, r), np.full(E, t)), int(h))):
            gap = np.abs(np.delete(row, true) - row[true]).min()
            gaps[side].append(gap)
            if not gap > MIN_GAP:
                raise SystemExit("%s: %s sweep of test triple %d has a competitor %.3g from the true candidate (<= %g)"
                                 % (name, side, i, gap, MIN_GAP))
            known = allt[(allt[:, 1] == r) & (allt[:, 0] == h), 2] if side == "tail" else allt[(allt[:, 1] == r) & (allt[:, 2] == t), 0]
            rank, frank = cr.rank64(row, true, known)
            want = (int(rec["eval.rank_%s" % side][i]), int(rec["eval.frank_%s" % side][i]))
            if (rank, frank) != want:
                raise SystemExit("%s: float64 %s ranks of test triple %d are %s, the reference recorded %s" % (name, side, i, (rank, frank), want))
    print("%s: smallest neighbour gap %.3g on head sweeps, %.3g on tail sweeps" % (name, min(gaps["head"]), min(gaps["tail"])))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (cls_path, hp, seed) in CASES.items():
        if only and name not in only:
            continue
        golden_with_fixed_filters(name, cls_path, hp, seed)
