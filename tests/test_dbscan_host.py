"""CPU-only checks of DBSCAN: header, ctypes binding and exported symbols agree; kge_dbscan refuses bad arguments before any GPU call
and its workspace query answers 0 for them; the workspace has no n^2 term; the wrappers and the Evaluator refuse bad arguments."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _call(lib, n=100, dim=8, stride=8, eps=1.0, min_samples=5, metric=0, rows=FAKE, ws=FAKE, ws_bytes=1 << 30, outs=(FAKE,) * 5):
    return lib.kge_dbscan(rows, n, dim, stride, eps, min_samples, metric, ws, ws_bytes, *outs, None)


BAD = [(dict(n=0), b"n = 0"), (dict(dim=0, stride=0), b"dim"), (dict(stride=7), b"row_stride"), (dict(eps=-1.0), b"eps"),
       (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(min_samples=0), b"min_samples"),
       (dict(metric=2), b"metric"), (dict(rows=None), b"null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace")] + \
      [(dict(outs=(FAKE,) * i + (None,) + (FAKE,) * (4 - i)), b"null") for i in range(5)]


@pytest.mark.parametrize("kw, word", BAD)
def test_dbscan_refuses_bad_arguments_without_gpu(kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) == -1
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_dbscan_header_binding_and_workspace_agree(monkeypatch):
    from pykg2vec_amd import _lib
    monkeypatch.delenv("KGE_DBS_SPLIT", raising=False)
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    lib = _lib.load()
    for sym in ("kge_dbscan_workspace_bytes", "kge_dbscan"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        proto = re.search(r"\b%s\(([^;]*)\);" % sym, text).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[sym][1]), sym
    assert {name: int(re.search(r"#define\s+KGE_DBS_%s\s+(\d+)" % name.upper(), text).group(1)) for name in _lib.DBS_METRICS} == _lib.DBS_METRICS
    for n, dim in ((0, 8), (100, 0), (1 << 31, 8)):
        assert lib.kge_dbscan_workspace_bytes(n, dim) == 0
    # no [n, n] block, bits included: six arrays of 4 bytes and one of 1 per row, and at most 64 slab partials of 4 bytes per row
    for n in (14951, 10 ** 6):
        assert 29 * n <= lib.kge_dbscan_workspace_bytes(n, 100) <= n * (64 * 4 + 25) + 4096 < n * n // 8


def test_dbscan_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from pykg2vec_amd import _lib, kernels
    from pykg2vec_amd.evaluator import Evaluator
    x = torch.zeros(10, 4)
    with pytest.raises(_lib.KgeHipError):
        kernels.dbscan(x, 1.0, 5)
    ev = Evaluator.__new__(Evaluator)   # its refusals come before any device or model access
    ev.config = types.SimpleNamespace(device="cpu")
    calls = [lambda: kernels.dbscan(x, 1.0, 5, metric="dot"), lambda: kernels.dbscan(x, -1.0, 5), lambda: kernels.dbscan(x, float("nan"), 5),
             lambda: kernels.dbscan(x, 1.0, 0), lambda: kernels.dbscan(x[:0], 1.0, 5), lambda: ev.dbscan_vectors(x[0], 1.0)]
    calls += [lambda kw=kw: ev.dbscan_vectors(x, **kw) for kw in (dict(eps=-1.0), dict(eps=float("inf")), dict(eps=1.0, min_samples=0),
                                                                  dict(eps=1.0, metric="dot"))]
    calls += [lambda kw=kw: ev.suggest_eps(**kw) for kw in (dict(min_samples=1), dict(min_samples=10 ** 6), dict(quantile=1.5), dict(metric="dot"))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    for bad in (x.double(), x[0]):
        with pytest.raises(TypeError):
            kernels.dbscan(bad, 1.0, 5)
