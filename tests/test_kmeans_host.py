"""CPU-only checks of the k-means clustering: header, ctypes binding and exported symbols agree; every kge_kmeans_* entry point refuses
bad arguments before any GPU call; the wrappers refuse CPU tensors and bad shapes."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _call(lib, entry, n=100, dim=8, stride=8, k=5, cstride=8, max_iter=3, rows=FAKE, cent=FAKE, ws=FAKE, ws_bytes=1 << 30, label=FAKE,
          out=FAKE):
    if entry == "assign":
        return lib.kge_kmeans_assign(rows, n, dim, stride, cent, k, cstride, ws, ws_bytes, label, out, None)
    if entry == "update":
        return lib.kge_kmeans_update(rows, n, dim, stride, label, k, 0, cent, cstride, out, ws, ws_bytes, None)
    if entry == "run":
        return lib.kge_kmeans_run(rows, n, dim, stride, cent, k, cstride, 0, max_iter, label, out, out, out, out, ws, ws_bytes, None)
    return lib.kge_kmeans_seed(rows, n, dim, stride, k, cent, ws, ws_bytes, label, out, None)


BAD = [(dict(n=0), b"n = 0"), (dict(k=0), b"k = 0"), (dict(k=101), b"k = 101"), (dict(n=5000, k=4097), b"k = 4097"),
       (dict(dim=0, stride=0, cstride=0), b"dim"), (dict(stride=7), b"row_stride"), (dict(rows=None), b"null"), (dict(cent=None), b"null"),
       (dict(label=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace")]


REFUSED = [(e, kw, word) for e in ("assign", "update", "run", "seed") for kw, word in BAD] \
    + [(e, dict(cstride=7), b"centroid_stride") for e in ("assign", "update", "run")] + [("run", dict(max_iter=-1), b"max_iter")]


@pytest.mark.parametrize("entry, kw, word", REFUSED)
def test_kmeans_refuses_bad_arguments_without_gpu(entry, kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert _call(lib, entry, **kw) == -1
    assert word in lib.kge_last_error(), lib.kge_last_error()


def test_kmeans_header_binding_and_constants_agree():
    from pykg2vec_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    assert int(re.search(r"#define\s+KGE_KMEANS_MAX_K\s+(\d+)", text).group(1)) == _lib.KMEANS_MAX_K == kernels.KMEANS_MAX_K == 4096
    assert int(re.search(r"#define\s+KGE_KMEANS_CHUNK\s+(\d+)", text).group(1)) == _lib.KMEANS_CHUNK == kernels.KMEANS_CHUNK
    lib = _lib.load()
    for sym in ("kge_kmeans_workspace_bytes", "kge_kmeans_assign", "kge_kmeans_update", "kge_kmeans_run", "kge_kmeans_seed"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        proto = re.search(r"\b%s\(([^;]*)\);" % sym, text).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[sym][1]), sym
    assert _lib.ABI_VERSION == 3   # additive entry points
    assert lib.kge_kmeans_workspace_bytes(10, 8, 11) == 0 and lib.kge_kmeans_workspace_bytes(14951, 100, 1000) >= 4 * (1000 + 2 * 14951)


def test_kmeans_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from pykg2vec_amd import _lib, kernels
    x, c = torch.zeros(10, 4), torch.zeros(3, 4)
    for call in (lambda: kernels.kmeans_assign(x, c), lambda: kernels.kmeans_run(x, c, 2), lambda: kernels.kmeans_seed(x, 3, torch.zeros(3).double()),
                 lambda: kernels.kmeans_update(x, torch.zeros(10, dtype=torch.int32), c)):
        with pytest.raises(_lib.KgeHipError):
            call()
    with pytest.raises(TypeError):
        kernels.kmeans_assign(x.double(), c)
    with pytest.raises(TypeError):
        kernels.kmeans_assign(x[0], c)
