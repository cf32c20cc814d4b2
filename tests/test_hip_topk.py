"""kge_topk_rows (csrc/kge_topk.hip) against the numpy restatement of its contract (tests/topk_ref.py: np.lexsort over id, key,
is-NaN, masked candidates dropped).  The order is total, so nothing here has a tolerance: ids and counts are compared with
array_equal and scores bit for bit.

Every (n_cand, dtype, direction) case runs ONE battery of 130 rows that cycles through the inputs that break a select -- random
normals, scores quantised to 8 levels (tie groups straddle the k-th place), a constant row, rows of +-0.0 and +-inf, rows with
NaNs, an all-NaN row -- through every k, three row counts, a strided view whose padding would win if it were read, and a mask
battery (no list, empty lists, unsorted lists with duplicates and out-of-range ids, lists holding keep[q], everything masked,
fewer live candidates than k)."""
import numpy as np
import pytest
import torch

import topk_ref

pytestmark = pytest.mark.gpu

N_CAND = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 14951]
KS = [1, 5, 64, 1000, 1024]
NQ = 130
DEV = "cuda"


def battery(n, dtype, seed):
    rng = np.random.default_rng(seed)
    rows = np.empty((NQ, n), dtype=np.float64)
    for q in range(NQ):
        kind = q % 8
        x = rng.normal(size=n)
        if kind == 1:
            x = np.floor(rng.random(n) * 8) / 4 - 1          # 8 levels, 0 among them
        elif kind == 2:
            x = np.full(n, 0.75)
        elif kind == 3:
            x = rng.choice([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], size=n)
        elif kind == 4:
            x[rng.random(n) < 0.3] = np.nan
        elif kind == 5:
            x = np.full(n, np.nan)
        elif kind == 6:
            x = np.where(rng.random(n) < 0.5, -0.0, 0.0)    # the two zeros only: one tie group whatever the sign bit
        elif kind == 7:
            x = np.round(x * 2) / 2
            x[rng.random(n) < 0.1] = -np.nan                # NaNs with the sign bit set
        rows[q] = x
    return rows.astype(dtype)


def orders(rows, largest):
    return [topk_ref.row_order(r, largest) for r in rows]


def pack(rows, order, k, live=None):
    nq = len(order)
    ids = np.full((nq, k), -1, dtype=np.int32)
    vals = np.full((nq, k), np.nan, dtype=rows.dtype)
    count = np.zeros(nq, dtype=np.int32)
    for q, o in enumerate(order):
        o = (o if live is None else o[live[q][o]])[:k]
        ids[q, :len(o)], vals[q, :len(o)], count[q] = o, rows[q, o], len(o)
    return ids, vals, count


def run(K, scores, k, largest, **kw):
    out = K.topk_rows(scores, k, largest=largest, **kw)
    return tuple(t.cpu().numpy() for t in out)


def skip_lists(n, seed):
    """(skip_off, skip_ids, keep) of the mask battery, one kind per row."""
    rng = np.random.default_rng(seed)
    lists, keep = [], np.full(NQ, -1, dtype=np.int64)
    for q in range(NQ):
        kind = q % 6
        if kind == 0:
            lst = np.empty(0, dtype=np.int64)
        elif kind == 1:                                       # unsorted, duplicates, ids outside [0, n)
            lst = np.concatenate([rng.integers(n, size=min(n, 40)), rng.integers(n, size=7).repeat(3), [-1, n, n + 5]])
            lst = lst[rng.permutation(len(lst))]
        elif kind == 2:                                       # holds keep[q]
            lst = rng.permutation(n)[:max(1, n // 3)]
            keep[q] = lst[len(lst) // 2]
        elif kind == 3:                                       # everything masked
            lst = rng.permutation(n)
        elif kind == 4:                                       # everything but three (or fewer) candidates: live < k for most k
            lst = rng.permutation(n)[:max(0, n - 3)]
        else:                                                 # everything masked but the kept one; keep of a row that lists nothing else
            lst = np.arange(n)[::-1]
            keep[q] = rng.integers(n)
        lists.append(lst.astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, np.concatenate(lists).astype(np.int32), keep


@pytest.fixture(scope="module")
def K():
    from pykg2vec_amd import kernels
    return kernels


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", N_CAND)
def test_select_matches_the_total_order(K, n, dtype, largest):
    rows = battery(n, dtype, seed=n)
    order = orders(rows, largest)
    dev = torch.from_numpy(rows).to(DEV)
    for k in KS:                                  # k > n_cand included: the rows are padded
        for nq in (1, 3, NQ):
            topk_ref.assert_same(run(K, dev[:nq], k, largest), pack(rows[:nq], order[:nq], k))
    # a view with row_stride = n + 37 whose padding holds the value that would win
    wide = torch.full((NQ, n + 37), float("inf") if largest else float("-inf"), dtype=dev.dtype, device=DEV)
    wide[:, :n] = dev
    view = wide[:, :n]
    assert view.stride(0) == n + 37
    for k in (5, 1024):
        topk_ref.assert_same(run(K, view, k, largest), pack(rows, order, k))
    # masks
    off, ids, keep = skip_lists(n, seed=1000 + n)
    live = [topk_ref.live_mask(q, n, off, ids, keep) for q in range(NQ)]
    d_off, d_ids, d_keep = (torch.from_numpy(a).to(DEV) for a in (off, ids, keep))
    for k in KS:
        got = run(K, dev, k, largest, skip_off=d_off, skip_ids=d_ids, keep=d_keep)
        topk_ref.assert_same(got, pack(rows, order, k, live))
    assert (got[2][3::6] == 0).all() and (got[0][3::6] == -1).all()          # everything masked: count 0, all -1
    assert (got[2][5::6] == 1).all() and np.array_equal(got[0][5::6, 0], keep[5::6])
    # no keep array; empty lists only (a null-sized id array)
    none_kept = [topk_ref.live_mask(q, n, off, ids, None) for q in range(NQ)]
    topk_ref.assert_same(run(K, dev, 5, largest, skip_off=d_off, skip_ids=d_ids), pack(rows, order, 5, none_kept))
    empty_off = torch.zeros(NQ + 1, dtype=torch.int64, device=DEV)
    empty_ids = torch.empty(0, dtype=torch.int32, device=DEV)
    topk_ref.assert_same(run(K, dev, 5, largest, skip_off=empty_off, skip_ids=empty_ids, keep=d_keep), pack(rows, order, 5))
    # two calls on the same inputs: identical bytes
    again = run(K, dev, 1000, largest, skip_off=d_off, skip_ids=d_ids, keep=d_keep)
    first = run(K, dev, 1000, largest, skip_off=d_off, skip_ids=d_ids, keep=d_keep)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def test_wrapper_refuses_what_the_library_cannot_take(K):
    x = torch.zeros((4, 10), device=DEV)
    with pytest.raises(ValueError, match="KGE_TOPK_MAX"):
        K.topk_rows(x, 1025)
    with pytest.raises(ValueError, match="inner stride"):
        K.topk_rows(torch.zeros((4, 20), device=DEV)[:, ::2], 3)
    with pytest.raises(TypeError):
        K.topk_rows(x.half(), 3)
    with pytest.raises(Exception, match="row_stride"):
        K.topk_rows(x[:1].expand(4, 10), 3)
    ids, vals, count = K.topk_rows(x[:0], 3)
    assert tuple(ids.shape) == (0, 3) and count.numel() == 0
