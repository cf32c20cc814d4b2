"""CPU-only: the MR / MRR / Hits arithmetic exists once (evaluator.rank_metrics) and MetricCalculator.settle and
Evaluator.test_relations both report exactly its numbers."""
import types

import numpy as np
import torch

from test_relations_host import _setup

HEAD, TAIL, HITS = [0, 1], [3, 9], [1, 3, 10]           # 0-based ranks; 1-based: 1, 2, 4, 10
MR = np.float32(4.25)
MRR = np.mean(np.reciprocal(np.array([1, 2, 4, 10], np.float32)))
HIT = {1: 0.25, 3: 0.5, 10: 1.0}


def test_rank_metrics_settle_and_test_relations_report_the_same_numbers():
    from pykg2vec_amd.evaluator import MetricCalculator, rank_metrics
    mr, mrr, hit = rank_metrics(np.array(HEAD + TAIL, np.float32) + 1, HITS)
    assert mr == MR and mr.dtype == np.float32 and mrr == MRR and mrr.dtype == np.float32
    assert hit == HIT and all(v.dtype == np.float32 for v in hit.values())

    mc = MetricCalculator(types.SimpleNamespace(hits=HITS))
    mc.append_ranks(np.array([HEAD, TAIL, HEAD, TAIL]), epoch=7)
    mc.settle()
    assert mc.mr[7] == MR and mc.fmr[7] == MR and mc.mrr[7] == MRR and mc.fmrr[7] == MRR
    assert {k: mc.hit[(7, k)] for k in HITS} == HIT and {k: mc.fhit[(7, k)] for k in HITS} == HIT
    assert mc.get_curr_scores() == {'mr': MR, 'fmr': MR, 'mrr': MRR, 'fmrr': MRR}

    c, cfg, m, ev, B, fn, known = _setup()
    cfg.hits = HITS
    counts = torch.tensor([HEAD + TAIL, HEAD + TAIL, [0] * 4, [0] * 4], dtype=torch.int32)      # raw, filtered, ties, filtered ties
    B.rank_relations = lambda desc, triples, **kw: counts
    got = ev.test_relations(c.test[:4], 4)
    assert got == {'mr': MR, 'fmr': MR, 'mrr': MRR, 'fmrr': MRR, 'hits': HIT, 'fhits': HIT}
    assert got['mr'].dtype == np.float32 and got['mrr'].dtype == np.float32 and got['hits'][3].dtype == np.float32
