"""Freeze the LIVE reference's outputs for tests/test_aten_restatement.py -> tests/golden/ref_aten_step.npz (container only:
imports /root/reference through oracle/ref_shim.py).  Re-run: python oracle/make_golden_aten.py

MKL runs on its reproducible branch (test_aten_restatement.PINNED_ENV; set before torch loads MKL), so that the frozen bits are the
ones every x86 host computes; the restatement must equal the reference bit for bit before anything is written."""
import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "tests")]
import test_aten_restatement as T  # noqa: E402

assert {"MKL_CBWR": os.environ["MKL_CBWR"]} == T.PINNED_ENV
out = {"torch_version": np.array(torch.__version__), "mkl_cbwr": np.array(os.environ["MKL_CBWR"])}
for l1, opt_name in T.CASES:
    ref = T.run_reference(l1, opt_name)
    got = T.run_restatement(l1, opt_name)
    assert set(got) == set(ref) and all(np.array_equal(got[k], ref[k]) for k in ref), (l1, opt_name)
    for k, v in ref.items():
        out["%s_%s_%s" % ("l1" if l1 else "l2", opt_name, k)] = v
path = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_aten_step.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
