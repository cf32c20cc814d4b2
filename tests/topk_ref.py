"""The contract of kge_topk_rows (include/kge_hip.h) restated in numpy: the expected value of the select tests, and the select of
the CPU plumbing tests' injected backend."""
import numpy as np
import torch


def live_mask(q, n, skip_off=None, skip_ids=None, keep=None):
    """bool [n]: candidate c of row q is live unless it is in the row's skip list and differs from keep[q]."""
    live = np.ones(n, dtype=bool)
    if skip_off is not None:
        lst = np.asarray(skip_ids[int(skip_off[q]):int(skip_off[q + 1])], dtype=np.int64)
        live[lst[(lst >= 0) & (lst < n)]] = False
        if keep is not None and 0 <= int(keep[q]) < n:
            live[int(keep[q])] = True
    return live


def row_order(row, largest, live=None):
    """Candidate ids of one row in the total order: numbers before NaNs, better score first, lower id first among equals
    (np.lexsort's last key is the primary one); masked candidates dropped."""
    row = np.asarray(row)
    bad = np.isnan(row)
    key = np.where(bad, 0, -row if largest else row)
    order = np.lexsort((np.arange(len(row)), key, bad))
    return order if live is None else order[live[order]]


def topk_ref(scores, k, largest=False, skip_off=None, skip_ids=None, keep=None):
    """(ids int32 [nq, k], values [nq, k], count int32 [nq]) of a numpy [nq, n] array, as kge_topk_rows returns them."""
    scores = np.asarray(scores)
    nq, n = scores.shape
    ids = np.full((nq, k), -1, dtype=np.int32)
    vals = np.full((nq, k), np.nan, dtype=scores.dtype)
    count = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        order = row_order(scores[q], largest, live_mask(q, n, skip_off, skip_ids, keep))[:k]
        m = len(order)
        ids[q, :m], vals[q, :m], count[q] = order, scores[q, order], m
    return ids, vals, count


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_same(got, want):
    """ids and counts equal, live scores bit for bit, padding NaN."""
    (gi, gv, gc), (wi, wv, wc) = got, want
    assert np.array_equal(gc, wc), (gc, wc)
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:8]
    live = wi >= 0
    assert np.array_equal(bits(gv)[live], bits(wv)[live])
    assert np.isnan(gv[~live]).all()
    assert np.array_equal(gv, wv, equal_nan=True)


def topk_rows_torch(scores, k, largest=False, skip_off=None, skip_ids=None, keep=None):
    """topk_ref with kernels.topk_rows's tensor interface (any device, strided rows): the select of a test backend."""
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    out = topk_ref(host(scores), int(k), bool(largest), host(skip_off), host(skip_ids), host(keep))
    return tuple(torch.from_numpy(a).to(scores.device) for a in out)
