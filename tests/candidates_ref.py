"""The contract of kge_rank_candidates / kge_rank_lists_from_scores (include/kge_hip.h) restated in numpy: the expected value of the
candidate-ranking tests, and the two calls of the CPU plumbing tests' injected backend."""
import numpy as np
import torch


def to_csr(table):
    """An integer [n, C] table (-1 = no entry) as (off int64 [n + 1], ids int32): every row is a list, padding included."""
    table = np.asarray(table)
    n, C = table.shape
    return np.arange(n + 1, dtype=np.int64) * C, table.reshape(-1).astype(np.int32)


def csr_of(lists):
    """Python lists of ids -> (off int64 [len + 1], ids int32)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ids = np.asarray([e for x in lists for e in x], dtype=np.int32).reshape(-1)
    return off, ids


def live_entries(triples, side, off, ids, list_of_query, E):
    """Per query the list entries that count: in [0, E) and not the true entity; duplicates kept, list order kept."""
    triples = np.asarray(triples)
    out = []
    for i in range(len(triples)):
        l = i if list_of_query is None else int(list_of_query[i])
        e = np.asarray(ids[int(off[l]):int(off[l + 1])], dtype=np.int64)
        true = int(triples[i, 0 if side else 2])
        out.append(e[(e >= 0) & (e < E) & (e != true)])
    return out


def expand(triples, side, entries):
    """(h, r, t, seg_off): the explicit triples of all entries (candidate in the swept column), query after query."""
    triples = np.asarray(triples, dtype=np.int64)
    cnt = np.asarray([len(e) for e in entries], dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    q = np.repeat(np.arange(len(triples)), cnt)
    e = np.concatenate(entries).astype(np.int64) if len(entries) and seg[-1] else np.zeros(0, np.int64)
    h = e if side else triples[q, 0]
    t = triples[q, 2] if side else e
    return np.ascontiguousarray(h), np.ascontiguousarray(triples[q, 1]), np.ascontiguousarray(t), seg


def kept_flags(entries, skip_off, skip_ids):
    """Per query a bool array over its live entries: not in the query's skip segment (any order, duplicates allowed)."""
    out = []
    for i, e in enumerate(entries):
        if skip_off is None:
            out.append(np.ones(len(e), dtype=bool))
        else:
            known = np.asarray(skip_ids[int(skip_off[i]):int(skip_off[i + 1])], dtype=np.int64)
            out.append(~np.isin(e, known))
    return out


def counts_from_scores(s_true, seg_scores, kept, largest=False):
    """int32 [4, n]: #better, #better and kept, #equal, #equal and kept per query (a NaN compares false both ways)."""
    n = len(s_true)
    out = np.zeros((4, n), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            s = np.asarray(seg_scores[i])
            better = (s > s_true[i]) if largest else (s < s_true[i])
            eq = s == s_true[i]
            out[:, i] = better.sum(), (better & kept[i]).sum(), eq.sum(), (eq & kept[i]).sum()
    return out


def rank_candidates_ref(score_fn, triples, side, off, ids, E, list_of_query=None, skip_off=None, skip_ids=None, largest=False):
    """int32 [4, n] of the contract, scores from score_fn(h, r, t) -> array (the composed path: expand, score, count)."""
    triples = np.asarray(triples, dtype=np.int64)
    entries = live_entries(triples, side, off, ids, list_of_query, E)
    h, r, t, seg = expand(triples, side, entries)
    s = np.asarray(score_fn(h, r, t)) if len(h) else np.zeros(0, np.float32)
    s_true = np.asarray(score_fn(triples[:, 0].copy(), triples[:, 1].copy(), triples[:, 2].copy()))
    segs = [s[seg[i]:seg[i + 1]] for i in range(len(triples))]
    return counts_from_scores(s_true, segs, kept_flags(entries, skip_off, skip_ids), largest)


def rank_lists_from_scores_ref(scores, truth, seg_off, flags=None, largest=False):
    scores, truth = np.asarray(scores), np.asarray(truth)
    n = len(truth)
    segs = [scores[int(seg_off[i]):int(seg_off[i + 1])] for i in range(n)]
    if flags is None:
        live = [np.ones(len(s), bool) for s in segs]
        kept = live
    else:
        f = np.asarray(flags)
        live = [(f[int(seg_off[i]):int(seg_off[i + 1])] & 1) != 0 for i in range(n)]
        kept = [l & ((f[int(seg_off[i]):int(seg_off[i + 1])] & 2) != 0) for i, l in enumerate(live)]
    return counts_from_scores(truth, [s[l] for s, l in zip(segs, live)], [k[l] for k, l in zip(kept, live)], largest)


def metrics(ranks, hits=(1, 3, 5, 10)):
    """MetricCalculator.settle's mr / fmr / mrr / fmrr from 0-based ranks [4, n] (head, tail, filtered head, filtered tail)."""
    ranks = np.asarray(ranks)
    r = np.concatenate([ranks[0], ranks[1]]).astype(np.float32) + 1
    f = np.concatenate([ranks[2], ranks[3]]).astype(np.float32) + 1
    return {"mr": np.mean(r), "fmr": np.mean(f), "mrr": np.mean(np.reciprocal(r)), "fmrr": np.mean(np.reciprocal(f))}


# ---- the two calls with kernels.py's tensor interface, for a test backend
_host = lambda t: None if t is None else t.detach().cpu().numpy()


def rank_candidates_torch(score_fn, E, triples, side, cand_off, cand_ids, list_of_query=None, skip_off=None, skip_ids=None, largest=False):
    out = rank_candidates_ref(score_fn, _host(triples), side, _host(cand_off), _host(cand_ids), E, _host(list_of_query), _host(skip_off),
                              _host(skip_ids), largest)
    return torch.from_numpy(out).to(triples.device)


def rank_lists_from_scores_torch(scores, truth_scores, seg_off, flags=None, largest=False):
    out = rank_lists_from_scores_ref(_host(scores), _host(truth_scores), _host(seg_off), _host(flags), largest)
    return torch.from_numpy(out).to(truth_scores.device)
