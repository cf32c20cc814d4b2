"""CPU-only checks of the PCA: header, ctypes binding and exported symbols agree; kge_pca_fit / kge_pca_transform refuse bad arguments
before any GPU call; the workspace has no [n, dim] term; the wrappers refuse bad arguments; the Evaluator hands the right rows on."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(256)   # never dereferenced: every refusal comes before the first GPU call


def _fit(lib, n=100, dim=8, stride=8, rows=FAKE, ws=FAKE, ws_bytes=1 << 30, outs=(FAKE,) * 6):
    return lib.kge_pca_fit(rows, n, dim, stride, ws, ws_bytes, *outs, None)


def _transform(lib, n=100, dim=8, stride=8, nc=2, ptrs=(FAKE,) * 5):
    return lib.kge_pca_transform(ptrs[0], n, dim, stride, *ptrs[1:4], nc, 0, ptrs[4], None)


BAD = [(_fit, dict(n=0), b"n = 0"), (_fit, dict(dim=0, stride=0), b"dim"), (_fit, dict(dim=513, stride=513), b"KGE_PCA_MAX_DIM"),
       (_fit, dict(stride=7), b"row_stride"), (_fit, dict(rows=None), b"null"), (_fit, dict(ws=None), b"workspace"),
       (_fit, dict(ws_bytes=16), b"workspace"), (_transform, dict(n=0), b"n = 0"), (_transform, dict(dim=513, stride=513), b"dim"),
       (_transform, dict(stride=7), b"row_stride"), (_transform, dict(nc=0), b"n_components"), (_transform, dict(nc=9), b"n_components")] + \
      [(_fit, dict(outs=(FAKE,) * i + (None,) + (FAKE,) * (5 - i)), b"null") for i in range(6)] + \
      [(_transform, dict(ptrs=(FAKE,) * i + (None,) + (FAKE,) * (4 - i)), b"null") for i in range(5)]


@pytest.mark.parametrize("call, kw, word", BAD)
def test_pca_refuses_bad_arguments_without_gpu(call, kw, word):
    from pykg2vec_amd import _lib
    lib = _lib.load()
    assert call(lib, **kw) == -1 and word in lib.kge_last_error(), lib.kge_last_error()


def test_pca_header_binding_and_workspace_agree(monkeypatch):
    from pykg2vec_amd import _lib, kernels
    monkeypatch.delenv("KGE_PCA_SPLIT", raising=False)
    text = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    lib = _lib.load()
    for sym in ("kge_pca_workspace_bytes", "kge_pca_fit", "kge_pca_transform"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
        proto = re.search(r"\b%s\(([^;]*)\);" % sym, text).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[sym][1]), sym
    assert int(re.search(r"#define\s+KGE_PCA_MAX_DIM\s+(\d+)", text).group(1)) == _lib.PCA_MAX_DIM == kernels.PCA_MAX_DIM == 512
    assert all(lib.kge_pca_workspace_bytes(n, dim) == 0 == kernels.pca_workspace_bytes(n, dim) for n, dim in ((0, 8), (100, 0), (100, 513), (1 << 31, 8)))
    assert lib.kge_pca_workspace_bytes(10 ** 6, 512) < 10 ** 6 * 512 * 4 // 8   # no [n, dim] temporary


def test_pca_wrappers_refuse_and_the_evaluator_hands_the_right_rows_on():
    from pykg2vec_amd import _lib, kernels
    from pykg2vec_amd.evaluator import Evaluator
    x, f64 = torch.zeros(10, 4), torch.float64
    good = kernels.PcaResult(torch.zeros(4, dtype=f64), None, torch.zeros(4, dtype=f64), torch.eye(4, dtype=f64), None, None)
    ev = Evaluator.__new__(Evaluator)   # its refusals come before any device or model access
    ev.config = types.SimpleNamespace(device="cpu")
    away = good._replace(mean=good.mean.to("meta"))
    refused = {_lib.KgeHipError: (lambda: kernels.pca_fit(x), lambda: kernels.pca_transform(x, good, 2)),   # no CPU fallback
               ValueError: (lambda: kernels.pca_fit(x[:1]), lambda: kernels.pca_fit(torch.zeros(4, 513)), lambda: kernels.pca_fit(torch.zeros(4, 0)),
                            lambda: kernels.pca_transform(x, good, 0), lambda: kernels.pca_transform(x, good, 5),
                            lambda: kernels.pca_transform(x[:, :3], good, 2), lambda: kernels.pca_transform(x, away, 2), lambda: ev.pca_vectors(x[0]),
                            lambda: ev.pca_vectors(x[:1]), lambda: ev.pca_vectors(x, 0), lambda: ev.pca_vectors(x, 5), lambda: ev.pca_transform_vectors(x)),
               TypeError: (lambda: kernels.pca_fit(x.double()), lambda: kernels.pca_fit(x[0]), lambda: kernels.pca_transform(x[0], good, 2),
                           lambda: kernels.pca_transform(x, good._replace(mean=good.mean.float()), 2))}
    for error, calls in refused.items():
        for call in calls:
            with pytest.raises(error):
                call()
    ent, rel, seen, lam = torch.arange(40.0).view(10, 4), torch.arange(12.0).view(3, 4), [], torch.tensor([3.0, 1.0, 0.0, 0.0], dtype=f64)
    ev.model = types.SimpleNamespace(entity_matrix=lambda tables: ent, relation_matrix=lambda tables: rel)
    ev.K = types.SimpleNamespace(   # a recording backend in place of the kernels layer
        pca_fit=lambda rows: seen.append(rows.clone()) or kernels.PcaResult(rows.double().mean(0), torch.diag(lam), lam, torch.eye(4, dtype=f64),
                                                                             torch.tensor([len(rows)]), torch.tensor([1])),
        pca_transform=lambda rows, fit, nc, whiten=False: seen.append((rows.clone(), fit, nc, whiten)) or rows[:, :nc])
    assert ev.last_pca is None and torch.equal(ev.pca_entities(3, ids=[4, 1], whiten=True), ent[[4, 1], :3])
    assert torch.equal(seen[0], ent[[4, 1]]) and torch.equal(seen[1][0], ent[[4, 1]]) and seen[1][2:] == (3, True)
    assert torch.equal(ev.last_pca.explained_variance_ratio, torch.tensor([0.75, 0.25, 0.0, 0.0], dtype=f64))
    assert torch.equal(ev.last_pca.mean, ent[[4, 1]].double().mean(0)) and int(ev.last_pca.count) == 2
    assert torch.equal(ev.pca_relations(), rel[:, :2]) and torch.equal(seen[2], rel) and seen[3][2:] == (2, False)
    assert torch.equal(ev.pca_transform_vectors(ent[:5].numpy(), 1), ent[:5, :1]) and seen[-1][1] is ev.last_pca and len(seen) == 5
    assert torch.equal(ev.pca_vectors(ent), ent[:, :2]) and torch.equal(seen[-2], ent)
