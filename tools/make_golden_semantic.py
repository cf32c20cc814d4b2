#!/usr/bin/env python
"""Freeze the LIVE reference's SLM / SME / SME_BL outputs into tests/golden/ref_{slm,sme,sme_bl}.npz (build container only:
oracle/make_golden.py imports the reference tree through oracle/ref_shim.py).  The recipe is oracle/make_golden.py's
golden_for, called unchanged: forward scores, loss and dense gradients of one hinge step, 3 steps x 4 optimisers,
Evaluator.test ranks and full sweeps.  Fixed seeds: a second run writes identical arrays.

Usage:  python tools/make_golden_semantic.py [slm|sme|sme_bl ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden  # noqa: E402

SEMANTIC = {
    "slm": ("pairwise.SLM", dict(ent_hidden_size=14, rel_hidden_size=10, margin=1.0), 3101),
    "sme": ("pairwise.SME", dict(hidden_size=16, margin=1.0), 3102),
    "sme_bl": ("pairwise.SME_BL", dict(hidden_size=16, margin=1.0), 3103),
}

if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (cls_path, hp, seed) in SEMANTIC.items():
        if not only or name in only:
            make_golden.golden_for(name, cls_path, hp, seed)
