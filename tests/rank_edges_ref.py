"""The numpy side of tests/test_hip_rank_edges.py: rank counts from a row of energies, and the query / known-triple sets whose sizes
sit on the rank passes' chunk, tile and threshold edges.  Plain numpy and python sets, no GPU.

The counts are golden_util.tie_bracket's and kge_oracle.rank_from_scores' (two statements of the same definition, checked against
each other here):
    rank          = #{e : s_e < s_true}
    filtered rank = rank - #{known e != true : s_e < s_true}
    ties          = #{e != true : s_e == s_true},   filtered ties = the same without the known entities
Rows that hold "higher is better" scores are negated by the caller first (negation is exact)."""
import numpy as np

import kge_oracle as ko
from golden_util import tie_bracket

CHUNK = 256          # kKg2eChunk = kSlmChunk = kNtnChunk: test triples per materialise-and-count chunk
LONG_LIST = 70       # known entities of the first and the last query of every chunk (more than one 64-wide tile of ids)


def counts(row, true_id, known=()):
    """(rank, filtered rank, ties, filtered ties) of the true candidate in one row of energies (lower = more plausible)."""
    row = np.asarray(row)
    less, ties, fless, fties = tie_bracket(row, int(true_id), known)
    assert (less, fless) == ko.rank_from_scores(row, int(true_id), known)
    return less, fless, ties, fties


def counts_all(rows, true_ids, known_lists):
    """int64 [4, n]: counts() of every row (rows [n, E]; known_lists: n iterables, or None = nothing known)."""
    n = len(true_ids)
    return np.asarray([counts(rows[i], true_ids[i], known_lists[i] if known_lists is not None else ()) for i in range(n)],
                      dtype=np.int64).reshape(n, 4).T


def distinct_queries(rng, n, E, R):
    """int64 [n, 3] triples whose (h, r) pairs are pairwise distinct and whose (r, t) pairs are too (n <= E * R); the extreme ids
    (0, 0, E - 1) and (E - 1, R - 1, 0) are queries 0 and 1."""
    assert 1 <= n <= E * R
    first = [(0, 0)] + ([(E - 1, R - 1)] if n > 1 and (E - 1, R - 1) != (0, 0) else [])
    codes = [h * R + r for h, r in first]
    rest = [c for c in rng.permutation(E * R).tolist() if c not in set(codes)]
    codes = (codes + rest)[:n]
    h, r = np.asarray(codes, dtype=np.int64) // R, np.asarray(codes, dtype=np.int64) % R
    t = np.empty(n, dtype=np.int64)
    for rel in range(R):
        idx = np.flatnonzero(r == rel)          # at most E of them: their heads are distinct
        pool = rng.permutation(E)
        if rel == 0:                            # query 0 takes tail E - 1 ...
            pool = np.concatenate([[E - 1], pool[pool != E - 1]])
        if rel == R - 1 and len(first) > 1:     # ... and query 1 tail 0 (each the first query of its relation)
            pool = np.concatenate([[0], pool[pool != 0]])
        t[idx] = pool[:len(idx)]
    q = np.stack([h, r, t], 1)
    assert len({(a, b) for a, b, _ in q.tolist()}) == n and len({(b, c) for _, b, c in q.tolist()}) == n
    assert tuple(q[0]) == (0, 0, E - 1) and (n < 2 or len(first) < 2 or tuple(q[1]) == (E - 1, R - 1, 0))
    return q


def known_triples(rng, q, E, R, background=None):
    """int64 [M, 3]: the queries but query 0, a random background and, by construction:
      * nothing known for (h_0, r_0): the tail list of query 0 is empty;
      * the head list of the last query holds every entity (but the true head where the last query is query 0);
      * the first and the last query of every CHUNK have min(LONG_LIST, E) known entities or more on both sides (query 0: heads only)."""
    n = len(q)
    h0, r0 = int(q[0, 0]), int(q[0, 1])
    m = 2 * n if background is None else background
    rows = [q[1:], np.stack([rng.integers(E, size=m), rng.integers(R, size=m), rng.integers(E, size=m)], 1)]
    last = n - 1
    h, r, t = (int(x) for x in q[last])
    rows.append(np.asarray([(e, r, t) for e in range(E) if not (last == 0 and e == h)], dtype=np.int64).reshape(-1, 3))
    for i in sorted({j for lo in range(0, n, CHUNK) for j in (lo, min(lo + CHUNK, n) - 1)}):
        h, r, t = (int(x) for x in q[i])
        ents = rng.permutation(E)[:min(LONG_LIST, E)]
        rows.append(np.asarray([(e, r, t) for e in ents], dtype=np.int64).reshape(-1, 3))
        rows.append(np.asarray([(h, r, e) for e in ents], dtype=np.int64).reshape(-1, 3))
    known = np.concatenate(rows).astype(np.int64)
    return np.ascontiguousarray(known[~((known[:, 0] == h0) & (known[:, 1] == r0))])


def known_lists(q, hr_t, tr_h):
    """(tail lists, head lists): per query the python set of known tails of (h, r) / known heads of (t, r)."""
    tails = [hr_t.get((int(h), int(r)), set()) for h, r, t in q]
    heads = [tr_h.get((int(t), int(r)), set()) for h, r, t in q]
    return tails, heads


def csr(lists):
    """(offsets int64 [n + 1], ids int32) of n python sets, ids ascending within a list."""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in lists])
    ids = np.asarray([e for s in lists for e in sorted(s)], dtype=np.int32).reshape(-1)
    return off, ids
