"""CPU-only checks of the silhouette: header, ctypes binding and exported symbols agree; kge_silhouette refuses bad arguments before any
GPU call and its workspace query answers 0 for them; the wrappers and the Evaluator refuse bad shapes, metrics and label ranges."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _call(lib, n=100, dim=8, stride=8, k=5, metric=0, rows=FAKE, label=FAKE, ws=FAKE, ws_bytes=1 << 30, outs=(FAKE,) * 6):
    return lib.kge_silhouette(rows, n, dim, stride, label, k, metric, ws, ws_bytes, *outs, None)


BAD = [(dict(n=1), b"n = 1"), (dict(dim=0, stride=0), b"dim"), (dict(k=1), b"k = 1"), (dict(k=4097), b"k = 4097"), (dict(stride=7), b"row_stride"),
       (dict(metric=2), b"metric"), (dict(rows=None), b"null"), (dict(label=None), b"null"), (dict(ws=None), b"workspace"),
       (dict(ws_bytes=16), b"workspace")] + [(dict(outs=(FAKE,) * i + (None,) + (FAKE,) * (5 - i)), b"null") for i in range(6)]


@pytest.mark.parametrize("kw, word", BAD)
def test_silhouette_refuses_bad_arguments_without_gpu(kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) == -1
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_silhouette_header_binding_and_workspace_agree(monkeypatch):
    from pykg2vec_amd import _lib
    monkeypatch.delenv("KGE_SIL_SPLIT", raising=False)
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    lib = _lib.load()
    for sym in ("kge_silhouette_workspace_bytes", "kge_silhouette"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        proto = re.search(r"\b%s\(([^;]*)\);" % sym, text).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[sym][1]), sym
    assert {name: int(re.search(r"#define\s+KGE_SIL_%s\s+(\d+)" % name.upper(), text).group(1)) for name in _lib.SIL_METRICS} == _lib.SIL_METRICS
    for n, dim, k in ((1, 8, 2), (100, 0, 2), (100, 8, 1), (100, 8, 4097)):
        assert lib.kge_silhouette_workspace_bytes(n, dim, k) == 0
    # no [n, n] block: rows, ranks, the padded member list and at most 64 slab partials of 20 bytes per row
    auto = lib.kge_silhouette_workspace_bytes(14951, 100, 1000)
    assert 4 * (4 * 14951 + 31 * 1000) <= auto <= 14951 * (64 * 20 + 64) + 1000 * 400
    # the switch SIL_SPLIT forces the number of slabs: 20 bytes of partials per row and slab, 64 slabs at the most
    sized = {}
    for split in (1, 3, 64, 1000):
        monkeypatch.setenv("KGE_SIL_SPLIT", str(split))
        sized[split] = lib.kge_silhouette_workspace_bytes(14951, 100, 1000)
    assert sized[1] <= auto <= sized[64] == sized[1000]
    assert all(abs(sized[s] - sized[1] - (s - 1) * 20 * 14951) <= 1024 for s in (3, 64))   # (up to the alignment of three arrays)


def test_silhouette_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from pykg2vec_amd import _lib, kernels
    from pykg2vec_amd.evaluator import Evaluator
    x, lab = torch.zeros(10, 4), torch.zeros(10, dtype=torch.int32)
    with pytest.raises(_lib.KgeHipError):
        kernels.silhouette(x, lab, 2)
    for call in (lambda: kernels.silhouette(x, lab, 2, metric="dot"), lambda: kernels.silhouette(x, lab, 1), lambda: kernels.silhouette(x, lab[:9], 2),
                 lambda: kernels.silhouette(x[:1], lab[:1], 2), lambda: kernels.silhouette(x, lab, 4097)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        kernels.silhouette(x.double(), lab, 2)
    ev = Evaluator.__new__(Evaluator)   # the refusals below come before any device or model access
    ev.config = types.SimpleNamespace(device="cpu")
    for labels, metric in ((np.zeros(10, np.int64), "l2"),            # one cluster: n_clusters = 1
                           (np.arange(10) - 2, "l2"),                 # a label below -1
                           (np.arange(10) * 1000, "l2"),              # n_clusters above KGE_KMEANS_MAX_K
                           (np.arange(9), "l2"), (np.arange(10) * 0.5, "l2"), (np.arange(10), "dot")):
        with pytest.raises(ValueError):
            ev.silhouette_vectors(x, labels, metric=metric)
    with pytest.raises(ValueError):
        ev.silhouette_vectors(x[0], np.arange(4))
    with pytest.raises(ValueError):
        ev.choose_n_clusters([1, 2])
