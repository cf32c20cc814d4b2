"""The contract of kge_rank_relations / kge_relation_csr_* (include/kge_hip.h) restated in numpy: the expected value of the
relation-ranking tests, and the calls of the CPU plumbing tests' injected backend."""
import numpy as np
import torch


def known_relations(known, queries):
    """Brute force: per query (h, ., t) the sorted distinct relations r with (h, r, t) in `known`, as python lists."""
    d = {}
    for h, r, t in np.asarray(known, dtype=np.int64).reshape(-1, 3).tolist():
        d.setdefault((h, t), set()).add(r)
    return [sorted(d.get((h, t), ())) for h, _, t in np.asarray(queries, dtype=np.int64).reshape(-1, 3).tolist()]


def csr_of(lists):
    """Python lists of ids -> (off int64 [len + 1], ids int32)."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ids = np.asarray([e for x in lists for e in x], dtype=np.int32).reshape(-1)
    return off, ids


def expand(triples, R):
    """(h, r, t) of the R - 1 OTHER relations of every query, query after query, relations ascending."""
    triples = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    n = len(triples)
    rel = np.tile(np.arange(R, dtype=np.int64), (n, 1))
    rel = rel[rel != triples[:, 1:2]].reshape(n, max(R - 1, 0))
    h = np.repeat(triples[:, 0], R - 1)
    t = np.repeat(triples[:, 2], R - 1)
    return np.ascontiguousarray(h), np.ascontiguousarray(rel.reshape(-1)), np.ascontiguousarray(t), rel


def counts_from_scores(s_true, s_other, rel, skip_off=None, skip_ids=None, largest=False):
    """int32 [4, n] from the scores [n, R - 1] of the other relations `rel` [n, R - 1]: #better, #better not in the skip segment,
    #equal, #equal not in the skip segment (a NaN compares false both ways; the segment may be in any order)."""
    n = len(s_true)
    out = np.zeros((4, n), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            s = np.asarray(s_other[i])
            kept = np.ones(len(s), dtype=bool)
            if skip_off is not None:
                kept = ~np.isin(rel[i], np.asarray(skip_ids[int(skip_off[i]):int(skip_off[i + 1])], dtype=np.int64))
            better = (s > s_true[i]) if largest else (s < s_true[i])
            eq = s == s_true[i]
            out[:, i] = better.sum(), (better & kept).sum(), eq.sum(), (eq & kept).sum()
    return out


def rank_relations_ref(score_fn, triples, R, skip_off=None, skip_ids=None, largest=False):
    """int32 [4, n] of the contract, scores from score_fn(h, r, t) -> array (the composed path: expand, score, count)."""
    triples = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    n = len(triples)
    h, r, t, rel = expand(triples, R)
    s = np.asarray(score_fn(h, r, t)).reshape(n, R - 1) if len(h) else np.zeros((n, 0), np.float32)
    s_true = (np.asarray(score_fn(triples[:, 0].copy(), triples[:, 1].copy(), triples[:, 2].copy())) if n else np.zeros(0, np.float32))
    return counts_from_scores(s_true, s, rel, skip_off, skip_ids, largest)


def metrics(ranks, hits=(1, 3, 5, 10)):
    """Evaluator.test_relations's dict from 0-based ranks [2, n] (raw, filtered): float32, as MetricCalculator.settle computes."""
    ranks = np.asarray(ranks)
    r = ranks[0].astype(np.float32) + 1
    f = ranks[1].astype(np.float32) + 1
    return {"mr": np.mean(r), "fmr": np.mean(f), "mrr": np.mean(np.reciprocal(r)), "fmrr": np.mean(np.reciprocal(f)),
            "hits": {k: np.mean(r <= k, dtype=np.float32) for k in hits}, "fhits": {k: np.mean(f <= k, dtype=np.float32) for k in hits}}


def same_metrics(a, b):
    return (set(a) == set(b) and all(a[k] == b[k] for k in ("mr", "fmr", "mrr", "fmrr")) and
            all(dict(a[k]) == dict(b[k]) for k in ("hits", "fhits")))


# ---- the call with kernels.py's tensor interface, for a test backend
_host = lambda t: None if t is None else t.detach().cpu().numpy()


def rank_relations_torch(score_fn, R, triples, skip_off=None, skip_ids=None, largest=False):
    out = rank_relations_ref(score_fn, _host(triples), R, _host(skip_off), _host(skip_ids), largest)
    return torch.from_numpy(out).to(triples.device)
