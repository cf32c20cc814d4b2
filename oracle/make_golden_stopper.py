"""Freeze the LIVE reference's early-stopping decisions for tests/test_host_cpu.py -> tests/golden/ref_early_stopper.npz
(container only: imports /root/reference through oracle/ref_shim.py).  Re-run: python oracle/make_golden_stopper.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tests")]
import ref_shim  # noqa: E402

ref_shim.install()
from pykg2vec.utils.trainer import EarlyStopper  # noqa: E402
from pykg2vec.common import Monitor  # noqa: E402
import test_host_cpu as T  # noqa: E402

seqs = T.patience_sequences()
stop = np.zeros(seqs.shape, dtype=bool)
for i, mon in enumerate(T.PATIENCE_MONITORS):
    for j, patience in enumerate(T.PATIENCE_VALUES):
        for trial in range(T.PATIENCE_TRIALS):
            ref = EarlyStopper(patience, Monitor(mon))
            for k, v in enumerate(seqs[i, j, trial]):
                stop[i, j, trial, k] = ref.should_stop({"mr": v, "fmr": v, "mrr": v, "fmrr": v})
path = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_early_stopper.npz")
np.savez_compressed(path, sequences=seqs, should_stop=stop)
print(path, os.path.getsize(path), "bytes")
