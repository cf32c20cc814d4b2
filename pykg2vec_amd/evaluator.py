"""Drop-in Evaluator / MetricCalculator (pykg2vec/utils/evaluator.py) on the fused rank sweep.

Same constructor `(model, config, tuning=False)`, same `mini_test / full_test / test / test_tail_rank /
test_head_rank` and `metric_calculator.{reset,settle,get_curr_scores,display_summary,save_test_summary}` surface
and dict fields, but `test()` ranks ALL requested triples in one kge_eval_ranks call: no per-triple id tensors, no
topk sort, no ordering copied to the host, no python rank loop.  The hr_t / tr_h dict-of-set caches are flattened
once into per-query CSR lists on the device.

Beyond the reference: `predict_tails / predict_heads / predict_rels` answer many queries per call, most plausible first, with
the known triples optionally left out (Model.score_rows + kernels.topk_rows); Trainer.infer_* is served by them.
`rank_candidates / test_candidates / test_type_constrained / test_sampled` rank every triple against a GIVEN list of candidates
(fixed negatives, type constraints, sampled ids) instead of all entities (kernels.rank_candidates; CandidateLists below).
`rank_relations / test_relations` rank the true RELATION of every triple among all relations, raw and with the relations known for
the pair (h, t) left out (kernels.rank_relations): MR / MRR / Hits@k of relation prediction.
`score_triples / classification_negatives / fit_thresholds / classify / test_classification` are triple classification: per-relation
thresholds fitted on labelled validation triples, then accuracy, per-relation accuracy and AUC (kernels.classification_fit /
classification_apply / corrupt_typed).
"""
import os
import timeit

import numpy as np
import torch

from . import kernels as K
from .kgmeta import ProjectionModel


def _log(msg):
    print(msg, flush=True)


def rank_metrics(ranks, hits):
    """(mr, mrr, {k: hits@k}) of 1-based float32 ranks, in float32 (evaluator.py:125-141)."""
    return np.mean(ranks), np.mean(np.reciprocal(ranks)), {k: np.mean(ranks <= k, dtype=np.float32) for k in hits}


def _summary_lines(title, second_line, mr, fmr, mrr, fmrr, hit, fhit, hits):
    lines = ["", title, second_line,
             "--mr,  filtered mr             : %.4f, %.4f" % (mr, fmr),
             "--mrr, filtered mrr            : %.4f, %.4f" % (mrr, fmrr)]
    for k in hits:
        lines.append("--hits%d                        : %.4f " % (k, hit[k]))
        lines.append("--filtered hits%d               : %.4f " % (k, fhit[k]))
    lines.append("---------------------------------------------------------")
    return lines


class MetricCalculator:
    """utils/evaluator.py:15-222, fed with rank arrays instead of candidate orderings."""

    def __init__(self, config):
        self.config = config
        try:  # the reference's dict-of-sets filters when the cache carries them ...
            self.hr_t = config.knowledge_graph.read_cache_data('hr_t')
            self.tr_h = config.knowledge_graph.read_cache_data('tr_h')
        except (KeyError, FileNotFoundError, AttributeError):  # ... else the flat splits are grouped on demand
            self.hr_t = self.tr_h = None
        self.mr, self.fmr, self.mrr, self.fmrr, self.hit, self.fhit = {}, {}, {}, {}, {}, {}
        self.epoch = None
        self.reset()

    def reset(self):
        self.rank_head, self.rank_tail, self.f_rank_head, self.f_rank_tail = [], [], [], []
        self.epoch = None
        self.start_time = timeit.default_timer()

    def append_ranks(self, ranks, epoch):
        """ranks: int array [4, n] = rank_head, rank_tail, filtered head, filtered tail (0-based)."""
        self.epoch = epoch
        self.rank_head = list(ranks[0])
        self.rank_tail = list(ranks[1])
        self.f_rank_head = list(ranks[2])
        self.f_rank_tail = list(ranks[3])

    def settle(self):  # evaluator.py:125-141
        head_ranks = np.asarray(self.rank_head, dtype=np.float32) + 1
        tail_ranks = np.asarray(self.rank_tail, dtype=np.float32) + 1
        head_franks = np.asarray(self.f_rank_head, dtype=np.float32) + 1
        tail_franks = np.asarray(self.f_rank_tail, dtype=np.float32) + 1
        self.mr[self.epoch], self.mrr[self.epoch], hit = rank_metrics(np.concatenate((head_ranks, tail_ranks)), self.config.hits)
        self.fmr[self.epoch], self.fmrr[self.epoch], fhit = rank_metrics(np.concatenate((head_franks, tail_franks)), self.config.hits)
        for k in self.config.hits:
            self.hit[(self.epoch, k)], self.fhit[(self.epoch, k)] = hit[k], fhit[k]

    def get_curr_scores(self):
        return {'mr': self.mr[self.epoch], 'fmr': self.fmr[self.epoch],
                'mrr': self.mrr[self.epoch], 'fmrr': self.fmrr[self.epoch]}

    def display_summary(self):
        dt = timeit.default_timer() - self.start_time
        e, hits = self.epoch, self.config.hits
        _log("\n".join(_summary_lines(
            "------Test Results for %s: Epoch: %s --- time: %.2f------------" % (getattr(self.config, "dataset_name", "?"), e, dt),
            "--# of entities, # of relations: %d, %d" % (self.config.tot_entity, self.config.tot_relation),
            self.mr[e], self.fmr[e], self.mrr[e], self.fmrr[e], {k: self.hit[(e, k)] for k in hits},
            {k: self.fhit[(e, k)] for k in hits}, hits)))

    def save_test_summary(self, model_name):
        """CSV of the per-epoch metrics, same columns as evaluator.py:186-206."""
        path = getattr(self.config, "path_result", None)
        if path is None:
            return
        import pandas as pd
        columns = ['Epoch', 'Mean Rank', 'Filtered Mean Rank', 'Mean Reciprocal Rank', 'Filtered Mean Reciprocal Rank']
        for hit in self.config.hits:
            columns += ['Hit-%d Ratio' % hit, 'Filtered Hit-%d Ratio' % hit]
        rows = []
        for epoch in self.mr:
            row = [epoch, self.mr[epoch], self.fmr[epoch], self.mrr[epoch], self.fmrr[epoch]]
            for hit in self.config.hits:
                row += [self.hit[(epoch, hit)], self.fhit[(epoch, hit)]]
            rows.append(row)
        n = len([f for f in os.listdir(str(path)) if model_name in f and 'Testing' in f])
        pd.DataFrame(rows, columns=columns).to_csv(os.path.join(str(path), "%s_Testing_results_%d.csv" % (model_name, n)))


def _as_array(data, n):
    """Triple objects (`.h .r .t`, data/kgcontroller.py:26-58) or an [N,3] array -> int64 [n,3]."""
    if n is None:
        n = len(data)
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data[:n], dtype=np.int64)
    return np.asarray([[data[i].h, data[i].r, data[i].t] for i in range(n)], dtype=np.int64).reshape(-1, 3)


def build_filter_csr(triples, hr_t, tr_h):
    """Flatten hr_t[(h,r)] / tr_h[(t,r)] (dict of sets) into per-query CSR: (tail_off, tail_ids, head_off, head_ids)."""
    n = triples.shape[0]
    t_off = np.zeros(n + 1, dtype=np.int64)
    h_off = np.zeros(n + 1, dtype=np.int64)
    t_ids, h_ids = [], []
    for i in range(n):
        h, r, t = int(triples[i, 0]), int(triples[i, 1]), int(triples[i, 2])
        a = hr_t.get((h, r), ())
        b = tr_h.get((t, r), ())
        t_ids.extend(a)
        h_ids.extend(b)
        t_off[i + 1] = t_off[i] + len(a)
        h_off[i + 1] = h_off[i] + len(b)
    return (t_off, np.asarray(t_ids, dtype=np.int32).reshape(-1), h_off, np.asarray(h_ids, dtype=np.int32).reshape(-1))


def _csr_side(queries_key, all_key, all_val):
    """Per query the unique values whose key equals the query's key: (offsets int64 [n+1], ids int32)."""
    pairs = np.unique(np.stack([all_key, all_val], 1), axis=0)          # sorted by key, then value; duplicates dropped
    ukeys, starts, counts = np.unique(pairs[:, 0], return_index=True, return_counts=True)
    pos = np.minimum(np.searchsorted(ukeys, queries_key), len(ukeys) - 1)
    found = ukeys[pos] == queries_key
    cnt = np.where(found, counts[pos], 0).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    # ids of query i = pairs[starts[pos[i]] : +cnt[i], 1]
    within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], cnt)
    ids = pairs[np.repeat(starts[pos], cnt) + within, 1].astype(np.int32)
    return off, ids


def build_filter_csr_from_triples(queries, known_triples, tot_relation):
    """The same CSR as build_filter_csr, straight from the flat splits: hr_t / tr_h are the tails / heads of
    train + valid + test grouped by (h, r) / (t, r) (data/kgcontroller.py:410-428); no dict of sets is materialised."""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    a = np.asarray(known_triples, dtype=np.int64).reshape(-1, 3)
    R = int(tot_relation)
    t_off, t_ids = _csr_side(q[:, 0] * R + q[:, 1], a[:, 0] * R + a[:, 1], a[:, 2])
    h_off, h_ids = _csr_side(q[:, 2] * R + q[:, 1], a[:, 2] * R + a[:, 1], a[:, 0])
    return t_off, t_ids, h_off, h_ids


def build_relation_csr_from_triples(queries, known_triples, tot_entity):
    """Per query (h, ., t) the distinct relations r with (h, r, t) in `known_triples` (train + valid + test), ascending, as a CSR:
    (rel_off int64 [n + 1], rel_ids int32).  The filter of relation ranking; hr_t / tr_h are keyed by (h, r) / (t, r) and cannot
    serve the pair key."""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    a = np.asarray(known_triples, dtype=np.int64).reshape(-1, 3)
    if a.shape[0] == 0:
        return np.zeros(q.shape[0] + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    E = int(tot_entity)
    off, ids = _csr_side(q[:, 0] * E + q[:, 2], a[:, 0] * E + a[:, 2], a[:, 1])
    return off.astype(np.int64), ids


class Evaluator:
    """utils/evaluator.py:225-334."""

    def __init__(self, model, config, tuning=False, backend=K):
        self.K = backend
        self.model = model
        self.config = config
        self.tuning = tuning
        self.test_data = config.knowledge_graph.read_cache_data('triplets_test')
        self.eval_data = config.knowledge_graph.read_cache_data('triplets_valid')
        self.metric_calculator = MetricCalculator(config)
        self._cache = {}
        self._groups = {}
        self._known_dev = None
        self.setup_stats = {}
        self.tie_counts = None     # [2, n] of the last test(): candidates tied with the true entity per head / tail sweep
        self._rel_cache = {}
        self.relation_tie_counts = None   # [n] of the last test_relations(): relations tied with the true relation
        self.thresholds = None     # ClassificationThresholds of the last fit_thresholds()
        self.n_dropped = 0         # rows the last classification_negatives() could not find a negative for
        self.last_projection_trace = None   # float64 [records, 2] = (KL, |grad|) of the last project_*() call

    # --- single-query hooks kept for Trainer.infer_* style callers (evaluator.py:249-273)
    def test_tail_rank(self, h, r, topk=-1):
        dev = self.config.device
        return self.model.predict_tail_rank(torch.as_tensor([int(h)], device=dev), torch.as_tensor([int(r)], device=dev),
                                            topk=topk).squeeze(0)

    def test_head_rank(self, r, t, topk=-1):
        dev = self.config.device
        return self.model.predict_head_rank(torch.as_tensor([int(t)], device=dev), torch.as_tensor([int(r)], device=dev),
                                            topk=topk).squeeze(0)

    def test_rel_rank(self, h, t, topk=-1):
        """evaluator.py:275-287: energies of (h, r, t) for every relation r through the batch scorer, then topk."""
        dev = self.config.device
        if hasattr(self.model, "predict_rel_rank"):
            return self.model.predict_rel_rank(torch.as_tensor([int(h)], device=dev), torch.as_tensor([int(t)], device=dev),
                                               topk=topk).squeeze(0)
        R = int(self.config.tot_relation)
        rel = torch.arange(R, dtype=torch.int64, device=dev)
        with torch.no_grad():
            preds = self.model.forward(torch.full((R,), int(h), dtype=torch.int64, device=dev), rel,
                                       torch.full((R,), int(t), dtype=torch.int64, device=dev))
        _, rank = torch.topk(preds, k=topk)
        return rank

    # --- batched link prediction: many queries per call, most plausible first, known triples optionally left out
    PREDICT_SCRATCH_BYTES = 256 << 20   # bound of the score rows held at once; a chunk is at least one row
    PREDICT_ROW_ITEM_BYTES = 8          # budgeted per score: float64 rows (MuRP), or the two float32 sides TransR / NTN / SLM sweep

    def _ids_arg(self, x, what):
        dev = self.config.device
        t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError("%s must be integer ids" % what)
        return t.reshape(-1).to(device=dev, dtype=torch.int64)

    def _topk_arg(self, topk):
        topk = int(topk)
        if not 1 <= topk <= K.TOPK_MAX:
            raise ValueError("topk = %d outside 1..%d (KGE_TOPK_MAX)" % (topk, K.TOPK_MAX))
        return topk

    def _select_chunks(self, n, n_cand, topk, rows_of, skip=None, keep=None):
        """rows_of(a, b) -> [b - a, n_cand] score rows of queries a..b; each chunk goes through topk_rows into ONE pair of output
        tensors.  Nothing in the loop reads the device."""
        dev = self.config.device
        ids = torch.empty((n, topk), dtype=torch.int64, device=dev)
        vals = None
        per = int(max(1, self.PREDICT_SCRATCH_BYTES // (self.PREDICT_ROW_ITEM_BYTES * n_cand)))
        for a in range(0, n, per):
            b = min(n, a + per)
            rows = rows_of(a, b)
            kw = {}
            if skip is not None:   # the chunk's offsets stay absolute: they index the whole id array
                kw = dict(skip_off=skip[0][a:b + 1], skip_ids=skip[1], keep=None if keep is None else keep[a:b])
            i, v, _ = self.K.topk_rows(rows, topk, largest=bool(self.model.higher_is_better), **kw)
            if vals is None:
                vals = torch.empty((n, topk), dtype=v.dtype, device=dev)
            ids[a:b] = i
            vals[a:b] = v
        if vals is None:
            vals = torch.empty((0, topk), dtype=torch.float32, device=dev)
        return ids, vals

    def _predict_entities(self, e, r, side, topk, filtered, keep):
        topk = self._topk_arg(topk)
        e, r = self._ids_arg(e, "tails" if side else "heads"), self._ids_arg(r, "relations")
        if e.numel() != r.numel():
            raise ValueError("%d entities for %d relations: one pair per query" % (e.numel(), r.numel()))
        n = int(e.numel())
        zero = torch.zeros_like(e)   # the swept column: a placeholder id
        queries = torch.stack([zero, r, e] if side else [e, r, zero], 1).contiguous()
        skip = None
        if keep is not None:
            keep = self._ids_arg(keep, "keep")
            if keep.numel() != n:
                raise ValueError("keep holds %d ids for %d queries" % (keep.numel(), n))
        if filtered and n:
            _, csr = self._filter_csr(queries.cpu().numpy(), queries)
            skip = (csr[2], csr[3]) if side else (csr[0], csr[1])
        return self._select_chunks(n, int(self.config.tot_entity), topk, lambda a, b: self.model.score_rows(queries[a:b], side), skip,
                                   keep if skip is not None else None)

    def predict_tails(self, h, r, topk=10, filtered=False, keep=None):
        """(ids int64 [n, topk], scores [n, topk]): the topk most plausible tails of every (h_i, r_i), most plausible first, equal
        scores by ascending id (kge_topk_rows).  h, r: ints, sequences or tensors of equal length.  filtered: the tails known for
        (h_i, r_i) in train + valid + test are left out, except keep[i] (an entity id per query: the true answer of a test triple).
        Rows with fewer than topk live candidates are padded with id -1 and a NaN score."""
        return self._predict_entities(h, r, 0, topk, filtered, keep)

    def predict_heads(self, r, t, topk=10, filtered=False, keep=None):
        """predict_tails for the heads of every (·, r_i, t_i)."""
        return self._predict_entities(t, r, 1, topk, filtered, keep)

    def predict_rels(self, h, t, topk=10):
        """(ids int64 [n, topk], scores [n, topk]): the topk most plausible relations of every (h_i, ·, t_i), all relations scored
        through the batch scorer.  The 1-N models' forward scores entities: they are refused, as the reference has no relation
        inference for them either."""
        if isinstance(self.model, ProjectionModel):
            raise ValueError("predict_rels: %s is a projection model, whose forward scores entities, not relations"
                             % type(self.model).__name__)
        topk = self._topk_arg(topk)
        h, t = self._ids_arg(h, "heads"), self._ids_arg(t, "tails")
        if h.numel() != t.numel():
            raise ValueError("%d heads for %d tails: one pair per query" % (h.numel(), t.numel()))
        R = int(self.config.tot_relation)
        rel = torch.arange(R, dtype=torch.int64, device=h.device)

        def rows_of(a, b):
            with torch.no_grad():
                return self.model.forward(h[a:b].repeat_interleave(R), rel.repeat(b - a), t[a:b].repeat_interleave(R)).view(b - a, R)

        return self._select_chunks(int(h.numel()), R, topk, rows_of)

    # --- nearest neighbours in embedding space: which entities / relations lie closest to given ones (kge_knn_rows)
    KNN_QUERY_BYTES = 8 * 2048 + 4   # most workspace kge_knn_rows takes per query: its partial lists (S * k <= 2048 pairs) and a norm

    def _knn_matrix(self, kind, tables):
        if kind not in ("entity", "relation"):
            raise ValueError("kind = %r (\"entity\" or \"relation\")" % (kind,))
        with torch.no_grad():
            m = self.model.entity_matrix(tables) if kind == "entity" else self.model.relation_matrix(tables)
        return m if m.stride(-1) == 1 else m.contiguous()

    def _knn_chunks(self, table, n, topk, metric, queries_of, self_ids=None):
        """queries_of(a, b) -> float32 [b - a, D] query rows a..b; the chunks are sized so that the search's workspace stays within
        PREDICT_SCRATCH_BYTES, and each goes through knn_rows into ONE pair of output tensors.  Nothing in the loop reads the device."""
        topk = int(topk)
        if not 1 <= topk <= K.KNN_MAX:
            raise ValueError("topk = %d outside 1..%d (KGE_KNN_MAX)" % (topk, K.KNN_MAX))
        K.knn_metric(metric)
        dev = table.device
        ids = torch.empty((n, topk), dtype=torch.int64, device=dev)
        vals = torch.empty((n, topk), dtype=torch.float32, device=dev)
        per = int(max(1, (self.PREDICT_SCRATCH_BYTES - 4 * int(table.shape[0])) // self.KNN_QUERY_BYTES))
        for a in range(0, n, per):
            b = min(n, a + per)
            i, v, _ = self.K.knn_rows(table, queries_of(a, b), topk, metric=metric, self_ids=None if self_ids is None else self_ids[a:b])
            ids[a:b] = i
            vals[a:b] = v
        return ids, vals

    def _nearest(self, kind, ids, topk, metric, tables, exclude_self):
        table = self._knn_matrix(kind, tables)
        ids = self._ids_arg(ids, "ids").to(table.device)
        return self._knn_chunks(table, int(ids.numel()), topk, metric, lambda a, b: table[ids[a:b]], ids if exclude_self else None)

    def nearest_entities(self, ids, topk=10, metric="cosine", tables=None, exclude_self=True):
        """(ids int64 [n, topk], scores float32 [n, topk]): the topk entities nearest to every entity of `ids` in embedding space,
        nearest first, equal scores by ascending id (kge_knn_rows).  metric: "cosine", "dot" (higher is nearer) or "l2" (the Euclidean
        distance).  The rows compared are Model.entity_matrix(tables).  exclude_self: entity ids[i] is not its own neighbour.  Rows
        with fewer than topk live candidates are padded with id -1 and a NaN score."""
        return self._nearest("entity", ids, topk, metric, tables, exclude_self)

    def nearest_relations(self, ids, topk=10, metric="cosine", tables=None, exclude_self=True):
        """nearest_entities over Model.relation_matrix(tables)."""
        return self._nearest("relation", ids, topk, metric, tables, exclude_self)

    def nearest_to_vectors(self, vectors, kind="entity", topk=10, metric="cosine", tables=None):
        """nearest_entities for query rows that are no rows of the table: `vectors` float32 [n, D] (or [D]) against the entity or
        relation matrix of D columns, e.g. ent[h] + rel[r] of a TransE.  Every row of the table is live."""
        table = self._knn_matrix(kind, tables)
        v = vectors.detach() if isinstance(vectors, torch.Tensor) else torch.as_tensor(np.asarray(vectors))
        v = v.to(device=table.device, dtype=torch.float32)
        v = v.view(1, -1) if v.dim() == 1 else v
        if v.dim() != 2 or v.shape[1] != table.shape[1]:
            raise ValueError("vectors %s against a %s matrix of %d columns" % (tuple(v.shape), kind, table.shape[1]))
        v = v if v.stride(-1) == 1 else v.contiguous()
        return self._knn_chunks(table, int(v.shape[0]), topk, metric, lambda a, b: v[a:b])

    def find_duplicates(self, kind="entity", metric="l2", threshold=None, topk=8, tables=None):
        """(pairs int64 [m, 2], scores float32 [m]): the pairs a < b of entities (or relations) whose score passes `threshold` --
        at most for "l2", at least for "cosine" / "dot" -- found among the topk nearest neighbours of every row; each pair once, in
        (a, b) order.  A pair's score is the same from either side (the sums run in the same order).  The search runs for every
        row in chunks that read nothing back; the filter runs once on the device behind them."""
        if threshold is None:
            raise ValueError("find_duplicates needs a threshold (a distance for \"l2\", a similarity for \"cosine\" / \"dot\")")
        table = self._knn_matrix(kind, tables)
        n = int(table.shape[0])
        own = torch.arange(n, dtype=torch.int64, device=table.device)
        ids, vals = self._knn_chunks(table, n, topk, metric, lambda a, b: table[a:b], own)
        passes = (vals <= float(threshold)) if metric == "l2" else (vals >= float(threshold))   # (NaN padding passes neither)
        a = own.view(-1, 1).expand_as(ids)
        key = torch.minimum(a, ids) * n + torch.maximum(a, ids)
        keep = passes & (ids >= 0)
        key, order = torch.sort(key[keep])
        score = vals[keep][order]
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]
        key, score = key[first], score[first]
        return torch.stack([key // n, key % n], 1), score

    # --- t-SNE projection of embedding rows to 2-D (kge_tsne_*): exact t-SNE over the sparse affinities of the neighbour search
    def _projection_init(self, X, init, seed):
        n = int(X.shape[0])
        if isinstance(init, torch.Tensor) or isinstance(init, np.ndarray):
            Y = torch.as_tensor(init).detach().to(device=X.device, dtype=torch.float32)
            if tuple(Y.shape) != (n, 2):
                raise ValueError("init must be [%d, 2] (got %s)" % (n, list(Y.shape)))
            return Y.clone().contiguous()
        if init == "random":
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(seed))
            return (1e-4 * torch.randn((n, 2), generator=gen, dtype=torch.float32)).to(X.device)
        if init != "pca":
            raise ValueError("init = %r (\"pca\", \"random\" or an [n, 2] tensor)" % (init,))
        # the top two principal axes of the D x D covariance; an eigenvector's sign is fixed by its largest component
        Xc = X.double() - X.double().mean(0, keepdim=True)
        _, vec = torch.linalg.eigh(Xc.t() @ Xc / max(n - 1, 1))
        top = vec[:, -2:].flip(1) if vec.shape[1] >= 2 else torch.cat([vec, torch.zeros_like(vec)], 1)
        big = top.gather(0, top.abs().argmax(0, keepdim=True))
        top = top * torch.where(big < 0, -torch.ones_like(big), torch.ones_like(big))
        Y = Xc @ top
        std = Y[:, 0].std(unbiased=False)
        Y = Y / torch.where(std > 0, std, torch.ones_like(std)) * 1e-4
        return Y.float().contiguous()

    def _project(self, X, perplexity=30.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250, learning_rate="auto",
                 init="pca", seed=0, record_every=50):
        n = int(X.shape[0])
        perplexity = float(perplexity)
        if n < 2:
            raise ValueError("a projection needs at least 2 rows (got %d)" % n)
        if not 1.0 <= perplexity < n:
            raise ValueError("perplexity = %g outside [1, n = %d)" % (perplexity, n))
        k = min(n - 1, int(3 * perplexity))
        if k > K.KNN_MAX:
            raise ValueError("perplexity = %g asks for %d neighbours per row, the search returns at most %d (KGE_KNN_MAX): "
                             "perplexity <= %d for more than %d rows" % (perplexity, k, K.KNN_MAX, K.KNN_MAX // 3, K.KNN_MAX + 1))
        n_iter, stop = int(n_iter), min(int(exaggeration_iter), int(n_iter))
        lr = max(n / float(early_exaggeration) / 4.0, 50.0) if isinstance(learning_rate, str) and learning_rate == "auto" else float(learning_rate)
        own = torch.arange(n, dtype=torch.int64, device=X.device)
        ids, dist = self._knn_chunks(X, n, k, "l2", lambda a, b: X[a:b], own)
        count = (ids >= 0).sum(1).to(torch.int32)
        cond_p, _ = self.K.tsne_affinities(ids, dist, count, perplexity)
        csr = self.K.tsne_joint(ids, cond_p, count)
        Y = self._projection_init(X, init, seed)
        update, gains = torch.zeros_like(Y), torch.ones_like(Y)
        Y, trace = self.K.tsne_run(csr, Y, stop, it0=0, exaggeration=float(early_exaggeration), momentum=0.5, learning_rate=lr,
                                   record_every=record_every, update=update, gains=gains,
                                   trace=torch.full((n_iter // record_every if record_every > 0 else 0, 2), float("nan"),
                                                    dtype=torch.float64, device=X.device))
        Y, trace = self.K.tsne_run(csr, Y, n_iter - stop, it0=stop, exaggeration=1.0, momentum=0.8, learning_rate=lr,
                                   record_every=record_every, update=update, gains=gains, trace=trace)
        self.last_projection_trace = trace
        return Y

    def _project_rows(self, kind, ids, tables, kw):
        table = self._knn_matrix(kind, tables)
        if ids is not None:
            table = table[self._ids_arg(ids, "ids").to(table.device)]
        return self._project(table if table.is_contiguous() else table.contiguous(), **kw)

    def project_entities(self, ids=None, tables=None, **kw):
        """float32 [n, 2] on the device: the t-SNE map of the entities `ids` (None: every entity), rows from
        Model.entity_matrix(tables).  Keywords and defaults are sklearn.manifold.TSNE's: perplexity=30.0, n_iter=1000,
        early_exaggeration=12.0, exaggeration_iter=250, learning_rate="auto" (max(n / early_exaggeration / 4, 50)), init="pca"
        ("random", or an [n, 2] tensor), seed=0; record_every=50 iterations (KL, |grad|) go to last_projection_trace.  The
        affinities are those of the min(n - 1, floor(3 perplexity)) nearest rows under L2 (nearest_entities' search), at most
        KGE_KNN_MAX: up to 129 rows the graph is complete and the result is exact t-SNE.  The descent is exact too (an all-pairs
        repulsion sweep, kge_tsne_run) and runs all n_iter iterations: there is no early stopping."""
        return self._project_rows("entity", ids, tables, kw)

    def project_relations(self, ids=None, tables=None, **kw):
        """project_entities over Model.relation_matrix(tables)."""
        return self._project_rows("relation", ids, tables, kw)

    def project_vectors(self, X, **kw):
        """project_entities for rows that are no table rows: X float32 [n, D], e.g. the concatenated h, r, t rows of a plot."""
        X = X.detach() if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
        X = X.to(device=self.config.device, dtype=torch.float32)
        if X.dim() != 2:
            raise ValueError("vectors must be [n, D] (got %s)" % (list(X.shape),))
        return self._project(X.contiguous(), **kw)

    def mini_test(self, epoch=None):
        n = len(self.eval_data) if self.config.test_num == 0 else min(self.config.test_num, len(self.eval_data))
        if self.config.debug:
            n = 10
        _log("Mini-Testing on [%d/%d] Triples in the valid set." % (n, len(self.eval_data)))
        return self.test(self.eval_data, n, epoch=epoch)

    def full_test(self, epoch=None):
        n = 10 if self.config.debug else len(self.test_data)
        _log("Full-Testing on [%d/%d] Triples in the test set." % (n, len(self.test_data)))
        return self.test(self.test_data, n, epoch=epoch)

    GROUPED_MIN_TRIPLES_PER_RELATION = 8  # measured crossover (Zipf-distributed test relations, FB15k shape): 8 beats 4 at 2k..32k triples

    def _dense_relations(self, trip):
        """Which test triples go through the per-relation candidate tables (kge_eval_ranks_grouped)?  TransR: all of them
        (its candidates only exist in a relation's space).  TransH / TransD: the triples of relations that have at least
        GROUPED_MIN_TRIPLES_PER_RELATION test triples -- there one transform of the candidate table per relation plus the
        plain sweep beats transforming every candidate for every query inside the sweep; rare relations keep the
        in-sweep transform.  Returns a bool mask over `trip`, or None when nothing is grouped."""
        name = getattr(self.model, "kernel_name", None)
        if name == "transr":
            return np.ones(len(trip), bool)
        if name in ("transh", "transd") and self.K is K and len(trip):
            counts = np.bincount(trip[:, 1], minlength=int(self.config.tot_relation))
            dense = counts[trip[:, 1]] >= self.GROUPED_MIN_TRIPLES_PER_RELATION
            return dense if dense.any() else None
        return None

    TABLE_BUDGET_BYTES = 1 << 30  # projected candidate tables held at once by a grouped TransR evaluation call

    def _group_chunks(self, trip, cuts):
        """Split the relation groups (runs of `trip`, boundaries `cuts`) into chunks whose candidate tables fit the
        budget; per chunk the device arrays kge_eval_ranks_grouped takes."""
        dev = next(self.model.parameters()).device
        dr = int(self.model.rel_hidden_size if self.model.kernel_name == "transr" else self.model.desc_kwargs()["dim"])
        table = ((int(self.config.tot_entity) + 63) // 64) * 64 * ((dr + 7) // 8 * 8) * 4
        per = int(max(1, min(4096, self.TABLE_BUDGET_BYTES // table)))
        chunks = []
        G = len(cuts) - 1
        for g0 in range(0, G, per):
            g1 = min(G, g0 + per)
            a, b = int(cuts[g0]), int(cuts[g1])
            cnt = np.diff(cuts[g0:g1 + 1])
            group_of_triple = np.repeat(np.arange(g1 - g0, dtype=np.int32), cnt)
            group_rel = trip[cuts[g0:g1], 1].astype(np.int64)
            nb = (2 * cnt + 15) // 16                       # sweep workgroups (16 queries each) per group
            blk_group = np.repeat(np.arange(g1 - g0, dtype=np.int64), nb)
            first_blk = np.concatenate([[0], np.cumsum(nb)[:-1]])
            within = np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(first_blk, nb)
            q_first = 2 * (cuts[g0:g1] - a)[blk_group] + 16 * within
            q_count = np.minimum(16, 2 * (cuts[g0 + 1:g1 + 1] - a)[blk_group] - q_first)
            qblocks = np.stack([blk_group, q_first, q_count, np.zeros_like(q_first)], 1).astype(np.int32)
            chunks.append((a, b, torch.from_numpy(group_of_triple).to(dev), torch.from_numpy(group_rel).to(dev),
                           torch.from_numpy(np.ascontiguousarray(qblocks)).to(dev)))
        return chunks

    DEVICE_CSR_MAX_ENTITY, DEVICE_CSR_MAX_RELATION = 1 << 24, 1 << 16   # packed key of kge_filter_csr_* (csrc/kge_index.hip)
    FILTER_SOURCE = None   # None: the rule of _filter_source; "triples" / "dicts": forced (tests compare the two)

    @staticmethod
    def _fingerprint(data, n):
        """Cache key of (data, n) by CONTENT: an `id()` can be reused by a different array after the first one is freed.
        Arrays: shape + per-column sums + an xor fold of the first n rows (tens of microseconds for 60 k rows); lists of Triple
        objects: length + the first, middle and last triple (walking 60 k python objects per call would cost more than the sweep)."""
        if isinstance(data, np.ndarray):
            a = np.ascontiguousarray(data[:n], dtype=np.int64)
            mix = a[:, 0] * 1000003 + a[:, 1] * 8191 + a[:, 2]
            return ("a", a.shape, int(a[:, 0].sum()), int(a[:, 1].sum()), int(a[:, 2].sum()),
                    int(np.bitwise_xor.reduce(mix)) if len(a) else 0)
        m = len(data) if n is None else n
        # 64 evenly spaced triples + the ends (a few microseconds): `id(data)` alone can be reused by a NEW list after the old one is
        # freed, and three samples would miss most edits; the id stays in the key only to keep distinct live lists apart cheaply
        pick = [data[i] for i in sorted({0, m - 1} | {(j * m) // 64 for j in range(64)})] if m else []
        return ("o", id(data), len(data), m, tuple((t.h, t.r, t.t) for t in pick))

    def _split_arrays(self):
        """[train, valid, test] as int64 [., 3] arrays; KeyError / FileNotFoundError / AttributeError when the cache lacks one."""
        kg = self.config.knowledge_graph
        return [_as_array(kg.read_cache_data(k), None) for k in ('triplets_train', 'triplets_valid', 'triplets_test')]

    def _known_triples(self):
        """train + valid + test as ONE int64 [M, 3] device tensor (what hr_t / tr_h are built from, data/kgcontroller.py:410-428),
        uploaded once per Evaluator; None when the cache does not carry the three splits."""
        if getattr(self, "_known_dev", None) is None:
            try:
                parts = self._split_arrays()
            except (KeyError, FileNotFoundError, AttributeError):
                return None
            dev = next(self.model.parameters()).device
            self._known_dev = torch.from_numpy(np.concatenate(parts)).to(dev)
        return self._known_dev

    def _filter_source(self):
        """Where the filter lists come from.  "triples": the three splits are numpy arrays in the cache -> sorted and searched on the
        device (kge_filter_csr_*; 1-2 ms for the FB15k test set).  "dicts": the reference's own cache format -- splits as lists of
        Triple objects next to the hr_t / tr_h dicts of sets: flattening the dicts for the evaluated queries on the host (a python
        loop, ~2 us per query) is then cheaper than converting ~600 k python objects into an array first."""
        if self.FILTER_SOURCE is not None:
            return self.FILTER_SOURCE
        if self.K is not K:
            return "dicts" if self.metric_calculator.hr_t is not None else "triples_host"
        kg = self.config.knowledge_graph
        try:
            flat = all(isinstance(kg.read_cache_data(k), np.ndarray) for k in ('triplets_train', 'triplets_valid', 'triplets_test'))
        except (KeyError, FileNotFoundError, AttributeError):
            flat = False
        if int(self.config.tot_entity) > self.DEVICE_CSR_MAX_ENTITY or int(self.config.tot_relation) > self.DEVICE_CSR_MAX_RELATION:
            # beyond the device builder's packed 24 / 16 / 24-bit key (csrc/kge_index.hip): the host builders have no such limit
            return "dicts" if self.metric_calculator.hr_t is not None else "triples_host"
        if flat or self.metric_calculator.hr_t is None:
            return "triples"
        return "dicts"

    def _filter_csr(self, trip, trip_dev):
        """(source, (tail_off, tail_ids, head_off, head_ids)) of the triples `trip` (host array) = `trip_dev` (device tensor): the
        known tails of every (h, r) and the known heads of every (t, r) over train + valid + test, from _filter_source()."""
        mc = self.metric_calculator
        dev = trip_dev.device
        source = self._filter_source()
        if source == "triples":   # sort + binary search on the device (csrc/kge_index.hip)
            known = self._known_triples()
            if known is None:
                raise K.L.KgeHipError("Evaluator: the knowledge-graph cache carries neither hr_t / tr_h nor the three splits")
            csr = self.K.filter_csr_build(known, trip_dev, self.config.tot_entity, self.config.tot_relation)
            if trip_dev.is_cuda:
                torch.cuda.synchronize(dev)
        elif source == "dicts":
            csr = tuple(torch.from_numpy(a).to(dev) for a in build_filter_csr(trip, mc.hr_t, mc.tr_h))
        else:  # host arrays without a device backend (CPU tests of the plumbing)
            known = np.concatenate(self._split_arrays())
            csr = tuple(torch.from_numpy(a).to(dev) for a in build_filter_csr_from_triples(trip, known, self.config.tot_relation))
        return source, tuple(csr)

    def _device_inputs(self, data, n):
        import time
        key = self._fingerprint(data, n)
        if key not in self._cache:
            t0 = time.perf_counter()
            trip = _as_array(data, n)
            dense = self._dense_relations(trip)
            if dense is not None:  # grouped triples first, sorted by relation; ranks are scattered back to the input order
                order = np.lexsort((trip[:, 1], ~dense))
                trip = np.ascontiguousarray(trip[order])
                nd = int(dense.sum())
                cuts = np.concatenate([[0], np.flatnonzero(np.diff(trip[:nd, 1])) + 1, [nd]]).astype(np.int64)
                self._groups[key] = (order, self._group_chunks(trip, cuts), nd)
            dev = next(self.model.parameters()).device
            trip_dev = torch.from_numpy(trip).to(dev)
            t1 = time.perf_counter()
            source, csr = self._filter_csr(trip, trip_dev)
            t2 = time.perf_counter()
            self.setup_stats = {"csr_ms": (t2 - t1) * 1e3, "csr_source": source, "queries": int(trip.shape[0]),
                                "host_prepare_ms": (t1 - t0) * 1e3, "filter_ids": int(csr[1].numel() + csr[3].numel())}
            self._cache[key] = (trip_dev,) + tuple(csr)
        return self._cache[key], key

    def _prepare_eval_tables(self):
        """What an evaluation does to the tables before it scores: RESCAL renormalises both, as the reference's forward does during
        eval too (pairwise.py:843-844)."""
        if getattr(self.model, "kernel_name", None) == "rescal":
            self.K.rescal_normalize(self.model.ent_embeddings.weight.data, self.model.rel_matrices.weight.data, self.model.hidden_size)

    def rank_all(self, data, n, return_ties=False):
        """int32 [4, n] device tensor of ranks for the first n triples of `data`.  return_ties: also an int32 [2, n] tensor (head
        sweeps, tail sweeps) with the number of OTHER candidates whose energy equals the true entity's bit for bit (the ranks are
        the optimistic end of such a tie group; -1 = not counted, None with a backend that does not count)."""
        (trip, t_off, t_ids, h_off, h_ids), key = self._device_inputs(data, n)
        self._prepare_eval_tables()
        desc = self.K.model_desc(self.model)
        count_ties = return_ties and self.K is K
        new_ties = lambda m: torch.zeros((2, m), dtype=torch.int32, device=trip.device) if count_ties else None
        kw = lambda t: {"ties": t} if count_ties else {}
        if key in self._groups:
            order, chunks, nd = self._groups[key]
            out = torch.empty((4, len(order)), dtype=torch.int32, device=trip.device)
            ties = new_ties(len(order))
            dst = torch.from_numpy(order).to(trip.device)
            if nd < len(order):  # rare relations: candidate transform inside the sweep
                t = new_ties(len(order) - nd)
                out[:, dst[nd:]] = self.K.eval_ranks(desc, trip[nd:], t_off[nd:], t_ids, h_off[nd:], h_ids, **kw(t))
                if count_ties:
                    ties[:, dst[nd:]] = t
            for a, b, got, grel, qb in chunks:  # many relation groups per launch, bounded by candidate-table memory
                t = new_ties(b - a)
                out[:, dst[a:b]] = self.K.eval_ranks_grouped(desc, trip[a:b], got, grel, qb, t_off[a:b + 1], t_ids,
                                                             h_off[a:b + 1], h_ids, **kw(t))
                if count_ties:
                    ties[:, dst[a:b]] = t
            return (out, ties) if return_ties else out
        ties = new_ties(trip.shape[0])
        # (the models with their own descriptor -- ConvKB, TuckER, ProjE_pointwise -- are told apart by K.eval_ranks)
        out = self.K.eval_ranks(desc, trip, t_off, t_ids, h_off, h_ids, **kw(ties))
        return (out, ties) if return_ties else out

    def test(self, data, num_of_test, epoch=None):
        self.metric_calculator.reset()
        ranks, ties = self.rank_all(data, num_of_test, return_ties=True)
        return self._settle(ranks, ties, epoch)

    def _settle(self, ranks, ties, epoch):
        """Ranks [4, n] (+ tie counts [2, n] or None) -> the MetricCalculator's summary dict, with the tie warning."""
        mc = self.metric_calculator
        ranks = ranks.cpu().numpy()  # the D2H copy: 4*n int32 (+ 2*n tie counts)
        self.tie_counts = ties.cpu().numpy() if ties is not None else None
        self._warn_ties(self.tie_counts, "entity")
        mc.append_ranks(ranks, epoch)
        mc.settle()
        mc.display_summary()
        if mc.epoch is not None and mc.epoch >= self.config.epochs - 1:
            mc.save_test_summary(self.model.model_name)
        return mc.get_curr_scores()

    @staticmethod
    def _warn_ties(t, what):
        if t is not None and (t > 0).any():
            # ranks are count-based (#candidates strictly below the true one): exact unless candidates TIE it, where the reference
            # lands somewhere inside the tie group (torch.topk's order) and this count is the optimistic end of it
            _log("WARNING: %d of %d rank sweeps have candidates whose energy equals the true %s's exactly (up to %d of them): the "
                 "reported ranks are the optimistic end of each tie group -- rank <= reference rank <= rank + ties; a saturated or "
                 "collapsed scorer (clamped energies, constant outputs) makes MR / MRR / Hits look better than they are"
                 % (int((t > 0).sum()), t.size, what, int(t.max())))

    # --- ranking against given candidates: the cost scales with the lists, not with tot_entity
    ROW_KERNEL_MODELS = frozenset(["transe", "transh", "transd", "transm", "rotate", "distmult", "complex", "analogy", "cp", "simple",
                                   "simple_ignr", "quate", "kg2e"])                       # the fused kernel (kge_rank_candidates)
    VIA_FORWARD_MODELS = frozenset(["rescal", "ntn", "transr", "slm", "sme", "sme_bl", "hole", "octonione", "convkb", "murp"])
    CANDIDATE_ENTRY_BYTES = 48   # budgeted per expanded list entry of the via-forward path: three int64 ids, a score, flags, indices

    def _candidate_lists(self, x, n, what):
        dev = self.config.device
        if isinstance(x, CandidateLists):
            lists = x.to(dev)
            if lists.list_of_query is None and lists.n_lists < n:
                raise ValueError("%s: %d lists for %d queries and no list_of_query" % (what, lists.n_lists, n))
            if lists.list_of_query is not None and lists.list_of_query.numel() < n:
                raise ValueError("%s: list_of_query holds %d entries for %d queries" % (what, lists.list_of_query.numel(), n))
            return lists
        t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        if t.dtype.is_floating_point or t.dtype == torch.bool or t.dim() != 2:
            raise TypeError("%s must be a CandidateLists or an integer [n, C] table (-1 = no entry)" % what)
        if t.shape[0] < n:
            raise ValueError("%s holds %d rows for %d queries" % (what, t.shape[0], n))
        C = int(t.shape[1])
        return CandidateLists(torch.arange(n + 1, dtype=torch.int64) * C, t[:n].reshape(-1)).to(dev)

    def _ranking_path(self, what, projection_note, no_path_note):
        """"rows" (the fused kernel) or "forward" (the model's own forward) for rank_candidates / rank_relations (`what`); the 1-N
        models and unknown ones are refused."""
        name = getattr(self.model, "kernel_name", None)
        if isinstance(self.model, ProjectionModel):
            raise ValueError("%s: %s is a projection model, %s" % (what, type(self.model).__name__, projection_note))
        if name not in self.ROW_KERNEL_MODELS and name not in self.VIA_FORWARD_MODELS:
            raise ValueError("%s: no %s path for model %r" % (what, no_path_note, name))
        return "rows" if name in self.ROW_KERNEL_MODELS else "forward"

    def _count_expanded(self, tq, h, r, t, seg, flags):
        """The shared tail of the via-forward paths: ONE forward call scores the m true triples `tq` and the expanded triples
        (h, r, t), whose segment of query i is seg[i] : seg[i + 1]; int32 [4, m] counts (rank_lists_from_scores)."""
        m = int(tq.shape[0])
        with torch.no_grad():
            s = self.model.forward(torch.cat([tq[:, 0], h]).contiguous(), torch.cat([tq[:, 1], r]).contiguous(),
                                   torch.cat([tq[:, 2], t]).contiguous()).reshape(-1)
        return self.K.rank_lists_from_scores(s[m:].contiguous(), s[:m].contiguous(), seg, flags,
                                             largest=bool(self.model.higher_is_better))

    def _rank_side_via_forward(self, trip, side, lists, skip_off, skip_ids):
        """int32 [4, n] counts of one side through the model's own forward: per chunk of queries the live list entries become
        explicit triples, ONE forward call scores the chunk's true triples and those, rank_lists_from_scores counts."""
        n = int(trip.shape[0])
        dev = trip.device
        E = int(self.config.tot_entity)
        col = 0 if side else 2
        out = torch.zeros((4, n), dtype=torch.int32, device=dev)
        loq = lists.list_of_query[:n] if lists.list_of_query is not None else torch.arange(n, dtype=torch.int64, device=dev)
        start = lists.off[loq]
        lens = (lists.off[loq + 1] - start).clamp_(min=0)
        lens_host = lens.cpu().numpy()   # the one host read: the chunk boundaries
        budget = max(1, self.PREDICT_SCRATCH_BYTES // self.CANDIDATE_ENTRY_BYTES)
        a = 0
        while a < n:
            b, tot = a + 1, int(lens_host[a])
            while b < n and tot + int(lens_host[b]) <= budget:
                tot += int(lens_host[b])
                b += 1
            m = b - a
            seg = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            seg[1:] = torch.cumsum(lens[a:b], 0)
            pos = torch.arange(tot, dtype=torch.int64, device=dev)
            qi = torch.searchsorted(seg, pos, right=True) - 1             # the chunk-local query of every entry
            e = lists.ids[start[a:b][qi] + pos - seg[qi]].to(torch.int64)
            tq = trip[a:b]
            live = (e >= 0) & (e < E) & (e != tq[qi, col])
            qi, e = qi[live], e[live]
            kept = torch.ones_like(e, dtype=torch.bool)
            if skip_off is not None and skip_ids.numel():
                lo, hi = skip_off[a], skip_off[b]
                spos = torch.arange(int(skip_ids.numel()), dtype=torch.int64, device=dev)
                sseg = torch.searchsorted(skip_off[a:b + 1].contiguous(), spos, right=True) - 1
                inside = (spos >= lo) & (spos < hi)
                keys = torch.sort((sseg * E + skip_ids.to(torch.int64))[inside]).values
                if keys.numel():
                    want = qi * E + e
                    at = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
                    kept = keys[at] != want
            live_seg = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            live_seg[1:] = torch.cumsum(torch.bincount(qi, minlength=m), 0)
            out[:, a:b] = self._count_expanded(tq, e if side else tq[qi, 0], tq[qi, 1], tq[qi, 2] if side else e, live_seg,
                                               (kept.to(torch.uint8) << 1) | 1)
            a = b
        return out

    def rank_candidates(self, data, n, tail_candidates, head_candidates, return_ties=False):
        """int32 [4, n] in rank_all's row order (rank_head, rank_tail, filtered head, filtered tail; 0-based) of the first n triples
        of `data`, each ranked against ITS candidates only: tail_candidates / head_candidates are CandidateLists, or integer [n, C]
        tables with -1 for "no entry".  The true entity is always a candidate; list entries equal to it or outside [0, tot_entity) are
        ignored, duplicates count as often as they occur.  The filtered ranks leave out the entities known for the pair in train +
        valid + test (the filter lists of rank_all).  return_ties: also int32 [2, n] (head, tail) with the number of candidates
        whose score equals the true entity's bit for bit; the ranks are the optimistic end of such a group.
        The row-kernel models take the fused kernel (kge_rank_candidates); RESCAL, NTN, TransR, SLM, SME, SME_BL, HoLE, OctonionE,
        ConvKB and MuRP score the expanded lists through their own forward.  The 1-N models are refused: rank_all is their path."""
        path = self._ranking_path("rank_candidates", "whose scorer is 1-N over all entities; rank_all is its path", "candidate-list")
        trip_host = _as_array(data, n)
        n = int(trip_host.shape[0])
        dev = self.config.device
        trip = torch.from_numpy(trip_host).to(dev)
        sides = [self._candidate_lists(tail_candidates, n, "tail_candidates"), self._candidate_lists(head_candidates, n, "head_candidates")]
        source, (t_off, t_ids, h_off, h_ids) = self._filter_csr(trip_host, trip) if n else (None, (None,) * 4)
        skips = [(t_off, t_ids), (h_off, h_ids)]
        counts = []
        if path == "rows":
            desc = self.K.model_desc(self.model)
            for side in (0, 1):
                ls = sides[side]
                loq = ls.list_of_query[:n].contiguous() if ls.list_of_query is not None else None
                counts.append(self.K.rank_candidates(desc, trip, side, ls.off, ls.ids, list_of_query=loq, skip_off=skips[side][0],
                                                     skip_ids=skips[side][1], skip_sorted=source in ("triples", "triples_host")))
        else:
            self._prepare_eval_tables()
            for side in (0, 1):
                counts.append(self._rank_side_via_forward(trip, side, sides[side], *skips[side]) if n
                              else torch.zeros((4, 0), dtype=torch.int32, device=dev))
        ct, ch = counts
        ranks = torch.stack([ch[0], ct[0], ch[1], ct[1]])
        return (ranks, torch.stack([ch[2], ct[2]])) if return_ties else ranks

    def test_candidates(self, data, n, tail_candidates, head_candidates, epoch=None):
        """test() over given candidates: the same MetricCalculator summary (and tie warning) from rank_candidates' ranks.  The
        metrics are over each query's list + its true entity, so they are comparable only between runs that use the same lists."""
        self.metric_calculator.reset()
        ranks, ties = self.rank_candidates(data, n, tail_candidates, head_candidates, return_ties=True)
        return self._settle(ranks, ties, epoch)

    def type_constraints(self):
        """(range_lists, domain_lists) of the training split (build_type_constraints), built once per Evaluator."""
        if getattr(self, "_type_constraints", None) is None:
            train = _as_array(self.config.knowledge_graph.read_cache_data('triplets_train'), None)
            self._type_constraints = build_type_constraints(train, self.config.tot_relation)
        return self._type_constraints

    def test_type_constrained(self, data=None, n=None, epoch=None):
        """Type-constrained ranking (Krompass et al., 2015): every test triple's tail is ranked among the entities seen as tail of
        its relation in the training split (+ itself), its head among those seen as head; filtered as usual.  data: default the
        test split."""
        data = self.test_data if data is None else data
        rel = torch.from_numpy(_as_array(data, n)[:, 1].copy())
        ranges, domains = self.type_constraints()
        return self.test_candidates(data, n, ranges.for_queries(rel), domains.for_queries(rel), epoch=epoch)

    def test_sampled(self, data, n, num_candidates, seed=0, epoch=None):
        """Ranking against `num_candidates` uniform entity ids per query and side, drawn on the device from a torch.Generator seeded
        with `seed` (the same seed draws the same candidates).  The metrics are over num_candidates + 1 candidates (the draws
        and the true entity): they are NOT comparable with full ranks over all entities, only with runs of the same num_candidates."""
        m = len(data) if n is None else int(n)
        dev = torch.device(self.config.device)
        g = torch.Generator(device=dev)
        g.manual_seed(int(seed))
        E = int(self.config.tot_entity)
        tails = torch.randint(E, (m, int(num_candidates)), generator=g, device=dev, dtype=torch.int64)
        heads = torch.randint(E, (m, int(num_candidates)), generator=g, device=dev, dtype=torch.int64)
        return self.test_candidates(data, m, tails, heads, epoch=epoch)

    # --- relation ranking: the true relation of (h, r, t) among all relations, raw and with the relations known for (h, t) left out
    def _relation_csr(self, trip, trip_dev):
        """(rel_off, rel_ids) device tensors: per query the relations known for its pair (h, t) over train + valid + test, ascending.
        Built on the device (kge_relation_csr_*) with the real backend when the splits are there and the ids fit the packed key;
        otherwise with numpy from the splits."""
        E, R = int(self.config.tot_entity), int(self.config.tot_relation)
        if self.K is K and E <= self.DEVICE_CSR_MAX_ENTITY and R <= self.DEVICE_CSR_MAX_RELATION:
            known = self._known_triples()
            if known is not None:
                return self.K.relation_csr_build(known, trip_dev, E, R)
        try:
            parts = self._split_arrays()
        except (KeyError, FileNotFoundError, AttributeError):
            raise K.L.KgeHipError("Evaluator: relation ranking filters by the pair (h, t), which needs the three splits in the "
                                  "knowledge-graph cache (hr_t / tr_h are keyed by (h, r) / (t, r))")
        return tuple(torch.from_numpy(a).to(trip_dev.device) for a in build_relation_csr_from_triples(trip, np.concatenate(parts), E))

    def _relation_inputs(self, data, n):
        key = self._fingerprint(data, n)
        if key not in self._rel_cache:
            trip = _as_array(data, n)
            trip_dev = torch.from_numpy(trip).to(self.config.device)
            self._rel_cache[key] = (trip_dev,) + tuple(self._relation_csr(trip, trip_dev))
        return self._rel_cache[key]

    def _rank_relations_via_forward(self, trip, rel_off, rel_ids):
        """int32 [4, n] counts through the model's own forward: per chunk of queries the R - 1 other relations of each query become
        explicit triples, ONE forward call scores the chunk's true triples and those, rank_lists_from_scores counts."""
        n = int(trip.shape[0])
        dev = trip.device
        R = int(self.config.tot_relation)
        out = torch.zeros((4, n), dtype=torch.int32, device=dev)
        per = int(max(1, (self.PREDICT_SCRATCH_BYTES // self.CANDIDATE_ENTRY_BYTES) // max(1, R - 1)))
        others = torch.arange(R - 1, dtype=torch.int64, device=dev)
        off_host = rel_off.cpu().numpy()   # the one host read: which skip entries belong to a chunk
        for a in range(0, n, per):
            b = min(n, a + per)
            m = b - a
            tq = trip[a:b]
            rel = others.unsqueeze(0) + (others.unsqueeze(0) >= tq[:, 1:2]).to(torch.int64)     # [m, R - 1]: every relation but the true one
            known = torch.zeros((m, R), dtype=torch.bool, device=dev)
            lo, hi = int(off_host[a]), int(off_host[b])
            if hi > lo:
                ids = rel_ids[lo:hi].to(torch.int64)
                row = torch.searchsorted(rel_off[a:b + 1].contiguous(), torch.arange(lo, hi, dtype=torch.int64, device=dev), right=True) - 1
                ok = (ids >= 0) & (ids < R)
                known[row[ok], ids[ok]] = True
            kept = ~known.gather(1, rel) if R > 1 else known[:, :0]
            flags = ((kept.reshape(-1).to(torch.uint8) << 1) | 1).contiguous()          # bit 0 live (every other relation is), bit 1 kept
            seg = torch.arange(m + 1, dtype=torch.int64, device=dev) * (R - 1)
            out[:, a:b] = self._count_expanded(tq, tq[:, 0].repeat_interleave(R - 1), rel.reshape(-1), tq[:, 2].repeat_interleave(R - 1),
                                               seg, flags)
        return out

    def rank_relations(self, data, n, return_ties=False):
        """int32 [2, n] device tensor: the 0-based rank of the true relation of the first n triples of `data` among all relations
        (row 0), and with the OTHER relations known for the pair (h, t) in train + valid + test left out (row 1).  return_ties: also
        int32 [n], the number of other relations whose score equals the true one's bit for bit; the ranks are the optimistic end of
        such a group.  The row-kernel models take the fused kernel (kge_rank_relations); RESCAL, NTN, TransR, SLM, SME, SME_BL, HoLE,
        OctonionE, ConvKB and MuRP score the expanded triples through their own forward.  The 1-N models are refused."""
        path = self._ranking_path("rank_relations", "whose forward scores entities, not relations", "relation-ranking")
        trip, rel_off, rel_ids = self._relation_inputs(data, n)
        if path == "rows":
            counts = self.K.rank_relations(self.K.model_desc(self.model), trip, skip_off=rel_off, skip_ids=rel_ids, skip_sorted=True)
        else:
            self._prepare_eval_tables()
            counts = self._rank_relations_via_forward(trip, rel_off, rel_ids)
        ranks = torch.stack([counts[0], counts[1]])
        return (ranks, counts[2].clone()) if return_ties else ranks

    def test_relations(self, data=None, n=None, epoch=None):
        """Relation prediction metrics over the first n triples of `data` (default: the test split): {'mr', 'fmr', 'mrr', 'fmrr',
        'hits': {k: .}, 'fhits': {k: .}} over config.hits, in float32 as MetricCalculator.settle computes the entity metrics, over the
        one relation side.  Logs a summary and the tie warning; the tie counts stay in `relation_tie_counts`."""
        data = self.test_data if data is None else data
        t0 = timeit.default_timer()
        ranks, ties = self.rank_relations(data, n, return_ties=True)
        ranks = ranks.cpu().numpy()
        self.relation_tie_counts = ties.cpu().numpy()
        self._warn_ties(self.relation_tie_counts, "relation")
        mr, mrr, hit = rank_metrics(ranks[0].astype(np.float32) + 1, self.config.hits)
        fmr, fmrr, fhit = rank_metrics(ranks[1].astype(np.float32) + 1, self.config.hits)
        _log("\n".join(_summary_lines(
            "------Relation Prediction Results for %s: Epoch: %s --- time: %.2f------------" % (
                getattr(self.config, "dataset_name", "?"), epoch, timeit.default_timer() - t0),
            "--# of triples, # of relations : %d, %d" % (ranks.shape[1], self.config.tot_relation),
            mr, fmr, mrr, fmrr, hit, fhit, self.config.hits)))
        return {'mr': mr, 'fmr': fmr, 'mrr': mrr, 'fmrr': fmrr, 'hits': hit, 'fhits': fhit}

    # --- triple classification (Socher et al. 2013): true or false, by the score against a per-relation threshold fitted on
    # labelled validation triples; accuracy, per-relation accuracy, AUC
    CLASSIFY_FORWARD_CHUNK = 1 << 20     # triples per forward call of score_triples
    CLASSIFY_MAX_DROPPED = 0.01          # share of negatives the bounded redraw may fail to produce before it is an error

    def _triples_arg(self, data, n=None):
        if isinstance(data, torch.Tensor):
            t = data.detach().reshape(-1, 3)[:n]
            if t.dtype.is_floating_point or t.dtype == torch.bool:
                raise TypeError("triples must be integer ids")
            return t.to(device=self.config.device, dtype=torch.int64).contiguous()
        return torch.from_numpy(_as_array(data, n)).to(self.config.device)

    def score_triples(self, triples):
        """float32 [n] on the device: the model's score of every (h, r, t) of `triples` [n, 3], through its own forward in chunks (the
        values forward returns, bit for bit; RESCAL renormalises its tables first, as every evaluation of it does).  The projection
        models score entities, not triples: their tail-side score_rows run in chunks bounded by PREDICT_SCRATCH_BYTES and the true
        tail's column is gathered."""
        trip = self._triples_arg(triples)
        n = int(trip.shape[0])
        out = torch.empty(n, dtype=torch.float32, device=trip.device)
        if isinstance(self.model, ProjectionModel):
            per = int(max(1, self.PREDICT_SCRATCH_BYTES // (self.PREDICT_ROW_ITEM_BYTES * int(self.config.tot_entity))))
            for a in range(0, n, per):
                b = min(n, a + per)
                out[a:b] = self.model.score_rows(trip[a:b], 0).gather(1, trip[a:b, 2:3]).reshape(-1)
            return out
        self._prepare_eval_tables()
        for a in range(0, n, self.CLASSIFY_FORWARD_CHUNK):
            b = min(n, a + self.CLASSIFY_FORWARD_CHUNK)
            with torch.no_grad():
                out[a:b] = self.model.forward(trip[a:b, 0].contiguous(), trip[a:b, 1].contiguous(), trip[a:b, 2].contiguous()).reshape(-1)
        return out

    def _classification_sampler(self):
        """(packed set of train + valid + test, type_off [2, R + 1], type_ids, bern table or None), built once per Evaluator."""
        if getattr(self, "_cls_sampler", None) is None:
            known = self._known_triples()
            if known is None:
                raise K.L.KgeHipError("Evaluator: classification negatives are filtered against train + valid + test, which needs the "
                                      "three splits in the knowledge-graph cache")
            dev = known.device
            ranges, domains = self.type_constraints()
            off = torch.stack([domains.off, ranges.off + int(domains.ids.numel())]).contiguous().to(dev)   # row 0 heads, row 1 tails
            ids = torch.cat([domains.ids, ranges.ids]).contiguous().to(dev)
            bern = None
            if getattr(self.config, "sampling", "uniform") == "bern":
                from .generator import bern_table, relation_property
                train = _as_array(self.config.knowledge_graph.read_cache_data('triplets_train'), None)
                bern = torch.from_numpy(bern_table(relation_property(train, self.config.tot_relation))).to(dev)
            self._cls_sampler = (self.K.triple_set_build(known), off, ids, bern)
        return self._cls_sampler

    def _draw_negatives(self, pos, seed, typed):
        """(neg int64 [n, 3] with -1 in the corrupted column of a failed row, number of failed rows) for the positives `pos`."""
        slots, off, ids, bern = self._classification_sampler()
        E, R = int(self.config.tot_entity), int(self.config.tot_relation)
        ph, pr, pt = (pos[:, i].contiguous() for i in range(3))
        if typed:
            neg, failed = self.K.corrupt_typed(ph, pr, pt, E, R, bern, off, ids, slots, seed, 0)
            return neg, int(failed.item())
        nh, nr, nt = self.K.corrupt(ph, pr, pt, 1, E, bern, slots, seed, 0)
        return torch.stack([nh, nr, nt], 1).contiguous(), 0

    def _labelled_pairs(self, data, n, negatives, seed, typed=True):
        """(positives [m, 3], negatives [m, 3], rows dropped): the first n triples of `data` with one negative each -- the given ones,
        or drawn.  A row whose bounded redraw failed is dropped together with its positive."""
        pos = self._triples_arg(data, n)
        if negatives is not None:
            neg = self._triples_arg(negatives)
            if neg.shape[0] != pos.shape[0]:
                raise ValueError("%d negatives for %d positives: one negative per positive" % (neg.shape[0], pos.shape[0]))
            return pos, neg, 0
        neg, failed = self._draw_negatives(pos, seed, typed)
        if failed:
            if failed > self.CLASSIFY_MAX_DROPPED * pos.shape[0]:
                raise K.L.KgeHipError("classification negatives: %d of %d positives found no negative within the bounded redraw (more than "
                                      "%g %%): the known-triple set leaves too little room" % (failed, pos.shape[0], 100 * self.CLASSIFY_MAX_DROPPED))
            keep = (neg >= 0).all(1)
            pos, neg = pos[keep].contiguous(), neg[keep].contiguous()
            _log("classification negatives: dropped %d of %d rows whose bounded redraw found no negative" % (failed, failed + pos.shape[0]))
        return pos, neg, failed

    def classification_negatives(self, data, n, seed=0, typed=True):
        """int64 [m, 3] on the device: one false triple per triple of the first n of `data`, head or tail replaced as the training
        sampler decides.  typed: the replacement comes from the entities seen on that side of the relation in the training split
        (Socher et al.'s protocol: a negative that is hard for the right reason), falling back to a uniform draw when the list runs
        out (kernels.corrupt_typed); else the training sampler's uniform draw (kernels.corrupt).  Either way a negative is never a
        known triple of train + valid + test, and a pure function of (seed, row).  Rows for which the bounded redraw found nothing are
        dropped (m < n, the count is logged and kept in `n_dropped`); more than CLASSIFY_MAX_DROPPED of the rows is an error."""
        _, neg, self.n_dropped = self._labelled_pairs(data, n, None, seed, typed)
        return neg

    def _labelled_scores(self, pos, neg):
        m = int(pos.shape[0])
        trip = torch.cat([pos, neg]).contiguous()
        label = torch.zeros(2 * m, dtype=torch.uint8, device=trip.device)
        label[:m] = 1
        return self.score_triples(trip), trip[:, 1].contiguous(), label

    def fit_thresholds(self, data=None, n=None, negatives=None, seed=0):
        """Fit, store in `self.thresholds` and return the per-relation thresholds (ClassificationThresholds) on the first n triples
        of `data` (default: the validation split) and one negative each (`negatives` [n, 3], default: classification_negatives with
        `seed`).  A relation without a triple there has seen == False and is classified by the global threshold, the fit of all the
        triples as one relation.  Exact: a threshold is an observed score, ties cut after the whole tie group, equal cuts -> the
        strictest (kernels.classification_fit)."""
        pos, neg, _ = self._labelled_pairs(self.eval_data if data is None else data, n, negatives, seed)
        scores, rel, label = self._labelled_scores(pos, neg)
        R, hib = int(self.config.tot_relation), bool(self.model.higher_is_better)
        thr, fit = self.K.classification_fit(scores, rel, label, R, higher_is_better=hib)
        gthr, gfit = self.K.classification_fit(scores, torch.zeros_like(rel), label, 1, higher_is_better=hib)
        self.thresholds = ClassificationThresholds(thr.cpu().numpy(), fit.cpu().numpy(), int(gthr.cpu()[0]), gfit.cpu().numpy()[0], hib)
        return self.thresholds

    def _apply_thresholds(self, scores, rel, label, th):
        dev = scores.device
        return self.K.classification_apply(scores, rel, torch.from_numpy(th.key).to(dev), torch.from_numpy(th.seen.astype(np.uint8)).to(dev),
                                           th.global_key, label=label, higher_is_better=th.higher_is_better)

    def classify(self, triples, thresholds=None):
        """bool [n] on the device: is (h, r, t) true under the thresholds (default: the stored ones, fitted on the validation split on
        first use)?"""
        th = thresholds or getattr(self, "thresholds", None) or self.fit_thresholds()
        trip = self._triples_arg(triples)
        pred, _ = self._apply_thresholds(self.score_triples(trip), trip[:, 1].contiguous(), None, th)
        return pred.to(torch.bool)

    def test_classification(self, data=None, n=None, negatives=None, seed=1, epoch=None):
        """Triple classification metrics over the first n triples of `data` (default: the test split) and one negative each: {'accuracy',
        'accuracy_per_relation' [R] (NaN without a test triple), 'auc', 'auc_per_relation' [R] (NaN without both labels), 'confusion'
        int64 [R, 4] = {tp, fp, tn, fn}, 'n_dropped'}.  Thresholds: the stored ones, fitted on the validation split on first use.  The
        AUC is threshold-free: (wins + ties / 2) / (positives * negatives) per relation, summed over relations, on the test scores."""
        t0 = timeit.default_timer()
        th = getattr(self, "thresholds", None) or self.fit_thresholds()
        pos, neg, dropped = self._labelled_pairs(self.test_data if data is None else data, n, negatives, seed)
        scores, rel, label = self._labelled_scores(pos, neg)
        _, conf = self._apply_thresholds(scores, rel, label, th)
        R = int(self.config.tot_relation)
        _, fit = self.K.classification_fit(scores, rel, label, R, higher_is_better=th.higher_is_better)
        conf, fit = conf.cpu().numpy(), fit.cpu().numpy()
        out = classification_metrics(conf, fit)
        out['n_dropped'] = dropped
        unseen = int(((conf.sum(1) > 0) & ~th.seen).sum())
        lines = ["", "------Triple Classification Results for %s: Epoch: %s --- time: %.2f------------" % (
            getattr(self.config, "dataset_name", "?"), epoch, timeit.default_timer() - t0),
            "--# of positives, # of relations        : %d, %d" % (pos.shape[0], R),
            "--relations on the global threshold     : %d" % unseen,
            "--dropped rows (no negative found)      : %d" % dropped,
            "--accuracy                              : %.4f" % out['accuracy'],
            "--mean per-relation accuracy            : %.4f" % (np.nanmean(out['accuracy_per_relation']) if conf.sum() else float('nan')),
            "--auc                                   : %.4f" % out['auc'],
            "---------------------------------------------------------"]
        _log("\n".join(lines))
        return out


def classification_key_to_score(key, higher_is_better):
    """float32 scores of classification keys (csrc/kge_classify_device.h), NaN where the key is -1 (no threshold)."""
    key = np.asarray(key, dtype=np.int64)
    k = (key & 0xFFFFFFFF).astype(np.uint32)
    asc = ~k if higher_is_better else k
    bits = np.where(asc & np.uint32(0x80000000), asc ^ np.uint32(0x80000000), ~asc).astype(np.uint32)
    out = bits.view(np.float32).copy()
    out[key < 0] = np.nan
    return out


class ClassificationThresholds:
    """Fitted classification thresholds as plain numpy (picklable): `key` int64 [R] in the key space of kge_classification_fit (-1 =
    nothing is positive), `value` float32 [R] the same as scores (a triple of relation r is true iff its score is at least as plausible
    as value[r]; NaN where key is -1), `seen` bool [R] (the relation had a validation triple; the others use `global_key` /
    `global_value`, the fit of all validation triples as one relation), `fit` int64 [R, 6] and `global_fit` [6] = {positives, negatives,
    correct at the cut, AUC wins, AUC ties, 0}, `higher_is_better` the orientation the keys were built with."""

    def __init__(self, key, fit, global_key, global_fit, higher_is_better):
        self.key = np.ascontiguousarray(key, dtype=np.int64)
        self.fit = np.ascontiguousarray(fit, dtype=np.int64)
        self.seen = (self.fit[:, 0] + self.fit[:, 1]) > 0
        self.global_key = int(global_key)
        self.global_fit = np.ascontiguousarray(global_fit, dtype=np.int64)
        self.higher_is_better = bool(higher_is_better)
        self.value = classification_key_to_score(self.key, self.higher_is_better)
        self.global_value = float(classification_key_to_score([self.global_key], self.higher_is_better)[0])


def classification_metrics(conf, fit):
    """The metrics dict of test_classification from conf int64 [R, 4] = {tp, fp, tn, fn} and the test scores' fit rows [R, 6]."""
    conf, fit = np.asarray(conf, dtype=np.int64), np.asarray(fit, dtype=np.int64)
    tot = conf.sum(1)
    right = conf[:, 0] + conf[:, 2]
    pairs = fit[:, 0] * fit[:, 1]
    twice = 2 * fit[:, 3] + fit[:, 4]       # 2 * (wins + ties / 2): integers until the one division
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'accuracy': float(right.sum()) / float(tot.sum()) if tot.sum() else float('nan'),
                'accuracy_per_relation': np.where(tot > 0, right / np.maximum(tot, 1), np.nan),
                'auc': float(twice.sum()) / float(2 * pairs.sum()) if pairs.sum() else float('nan'),
                'auc_per_relation': np.where(pairs > 0, twice / np.maximum(2 * pairs, 1), np.nan),
                'confusion': conf}


class CandidateLists:
    """Candidate lists as a CSR: list l = ids[off[l] : off[l + 1]] (off int64 [n_lists + 1], ids int32); query i uses list
    list_of_query[i], or list i when list_of_query is None.  Tensors or arrays; Evaluator moves them to its device."""

    def __init__(self, off, ids, list_of_query=None):
        as_t = lambda x, dt: (x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).reshape(-1).to(dt).contiguous()
        self.off, self.ids = as_t(off, torch.int64), as_t(ids, torch.int32)
        self.list_of_query = None if list_of_query is None else as_t(list_of_query, torch.int64)
        if self.off.numel() < 1:
            raise ValueError("off must hold n_lists + 1 offsets")

    @property
    def n_lists(self):
        return int(self.off.numel()) - 1

    def to(self, device):
        return CandidateLists(self.off.to(device), self.ids.to(device), None if self.list_of_query is None else self.list_of_query.to(device))

    def for_queries(self, list_of_query):
        """The same lists with query i mapped to list list_of_query[i] (type constraints: the queries' relation ids)."""
        return CandidateLists(self.off, self.ids, list_of_query)


def build_type_constraints(train_triples, tot_relation):
    """(range_lists, domain_lists): per relation r the unique tails / heads seen with r in `train_triples` [N, 3], ascending, as
    CandidateLists with one list per relation (a relation absent from the split has an empty list).  Use .for_queries(relation ids)."""
    a = np.asarray(train_triples, dtype=np.int64).reshape(-1, 3)
    R = int(tot_relation)
    rels = np.arange(R, dtype=np.int64)
    if a.shape[0] == 0:
        empty = lambda: CandidateLists(np.zeros(R + 1, np.int64), np.zeros(0, np.int32))
        return empty(), empty()
    t_off, t_ids = _csr_side(rels, a[:, 1], a[:, 2])
    h_off, h_ids = _csr_side(rels, a[:, 1], a[:, 0])
    return CandidateLists(t_off, t_ids), CandidateLists(h_off, h_ids)
