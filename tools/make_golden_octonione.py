#!/usr/bin/env python
"""Freeze the LIVE reference's OctonionE outputs into tests/golden/ref_octonione{,_neg3}.npz (build container only:
oracle/make_golden.py imports the reference tree through oracle/ref_shim.py).  The recipe is oracle/make_golden.py's
golden_for, called unchanged.  Fixed seeds: a second run writes identical arrays.

  octonione       hidden_size = 12, lmbda = 0.01, neg_rate 1 (the reference's default regulariser: N3, means over B * d)
  octonione_neg3  the same with neg_rate = 3: every positive is followed by three corruptions (bundles of four rows)

Usage:  python tools/make_golden_octonione.py [octonione|octonione_neg3 ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden  # noqa: E402

CASES = {
    "octonione": ("pointwise.OctonionE", dict(hidden_size=12, lmbda=0.01), 3301),
    "octonione_neg3": ("pointwise.OctonionE", dict(hidden_size=12, lmbda=0.01, neg_rate=3), 3302),
}

if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (cls_path, hp, seed) in CASES.items():
        if only and name not in only:
            continue
        make_golden.golden_for(name, cls_path, hp, seed)
