"""The contract of kge_knn_rows (include/kge_hip.h) restated in numpy, scores in float64: the expected value of the search tests and
the search of the CPU plumbing tests' injected backend.  The order is topk_ref.row_order's np.lexsort order."""
import numpy as np
import torch

import topk_ref

METRICS = ("dot", "cosine", "l2")


def scores64(table, queries, metric):
    """float64 [nq, n_rows]: dot, cosine (a zero-norm row: 0 to everything, NaN where an operand holds one) or Euclidean distance."""
    t, q = np.asarray(table, np.float64), np.asarray(queries, np.float64)
    with np.errstate(all="ignore"):
        if metric == "l2":
            return np.sqrt(((q[:, None, :] - t[None, :, :]) ** 2).sum(-1))
        dot = q @ t.T
        if metric == "dot":
            return dot
        den = np.sqrt((q * q).sum(1))[:, None] * np.sqrt((t * t).sum(1))[None, :]
        return np.where(den == 0, dot * 0.0, dot / np.where(den == 0, 1.0, den))


def knn_ref(table, queries, k, metric="cosine", self_ids=None, scores=None):
    """(ids int32 [nq, k], scores float64 [nq, k], count int32 [nq]) as kge_knn_rows returns them; `scores`: the block to select
    from instead of scores64's."""
    S = scores64(table, queries, metric) if scores is None else np.asarray(scores)
    nq, n = S.shape
    ids = np.full((nq, k), -1, dtype=np.int32)
    vals = np.full((nq, k), np.nan, dtype=S.dtype)
    count = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        live = np.ones(n, dtype=bool)
        if self_ids is not None and 0 <= int(self_ids[q]) < n:
            live[int(self_ids[q])] = False
        order = topk_ref.row_order(S[q], metric != "l2", live)[:k]
        m = len(order)
        ids[q, :m], vals[q, :m], count[q] = order, S[q, order], m
    return ids, vals, count


def knn_rows_torch(table, queries, k, metric="cosine", self_ids=None):
    """knn_ref with kernels.knn_rows's tensor interface and float32 scores: the search of a test backend."""
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    i, v, c = knn_ref(host(table), host(queries), int(k), metric, host(self_ids))
    return tuple(torch.from_numpy(a).to(table.device) for a in (i, v.astype(np.float32), c))
