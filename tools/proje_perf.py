#!/usr/bin/env python
"""Dev tool: the fused ProjE_pointwise step (kge_proje_train: labelled columns only) against the torch-ROCm eager restatement of the
reference's DENSE step on the same GPU (ATen: it forms the [B, E] logits, their sigmoid and the two masked log terms per direction),
at the yaml preset (k = 200, B = 200, dropout 0.5, FB15k shape), with and without the 100 negative labels.  Both versions are warmed
up and then timed in alternating rounds of 10 back-to-back steps between two events; the median of 7 rounds is reported with the
spread.  A round of the fused step is short (milliseconds): the spread column says what the figure is worth.
Usage: python tools/proje_perf.py > profiles/r11_proje_perf.txt"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.projection import ProjE_pointwise  # noqa: E402

E, R, D, B, P_DROP, LMBDA = 14951, 1345, 200, 200, 0.5, 1e-5
ROUNDS, INNER = 7, 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER * 1e3


def bench_pair(f, g, warm=5):
    """Median [min, max] microseconds per call of f and of g, their rounds alternating."""
    for _ in range(warm):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(ROUNDS):
        tf.append(timed(f))
        tg.append(timed(g))
    return [(statistics.median(x), min(x), max(x)) for x in (tf, tg)]


def eager_step(m, h, r, t, y1, y2):
    """models/projection.py:194-210 twice + get_reg + backward, dense labels, torch's own dropout."""
    ws = m.trainable_tensors()
    for p in ws:
        p.grad = None
    ent, rel, bc1, De1, Dr1, bc2, De2, Dr2 = ws
    zero = torch.zeros(1, device=ent.device)

    def fwd(e, y, De, Dr, bc):
        x = torch.dropout(torch.tanh(ent[e] * De + rel[r] * Dr + bc), p=P_DROP, train=True)
        s = torch.sigmoid(torch.matmul(x, ent.T))
        return (-torch.sum(torch.log(torch.clamp(s, 1e-10, 1.0)) * torch.max(zero, y))
                - torch.sum(torch.log(torch.clamp(1 - s, 1e-10, 1.0)) * torch.max(zero, torch.neg(y))))
    reg = LMBDA * (torch.sum(torch.abs(De1) + torch.abs(Dr1)) + torch.sum(torch.abs(De2) + torch.abs(Dr2)) + torch.sum(torch.abs(ent))
                   + torch.sum(torch.abs(rel)))
    (fwd(h, y1, De1, Dr1, bc1) + fwd(t, y2, De2, Dr2, bc2) + reg).backward()


def main():
    assert torch.cuda.is_available(), "proje_perf needs the GPU: a CPU timing says nothing"
    rng = np.random.default_rng(0)
    print("# fused ProjE_pointwise step vs eager ATen (dense labels), E = %d, R = %d, k = %d, B = %d, dropout %.1f; microseconds per step:"
          " median [min, max] of %d alternating rounds of %d steps" % (E, R, D, B, P_DROP, ROUNDS, INNER))
    m = ProjE_pointwise(tot_entity=E, tot_relation=R, hidden_size=D, lmbda=LMBDA, hidden_dropout=P_DROP).cuda()
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=1, offset=0)
    h, r, t = (torch.from_numpy(rng.integers(n, size=B)).cuda() for n in (E, R, E))
    per_row = 4      # positives per row and direction (FB15k's hr_t lists average a few entries)
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * per_row
    ids_np = np.sort(np.stack([rng.permutation(E)[:per_row] for _ in range(B)]), axis=1).astype(np.int32)
    ids = torch.from_numpy(ids_np.reshape(-1)).cuda()
    loss = K.new_loss_buffer(ws[0].device)
    for n_neg in (100, 0):
        neg_np = rng.permutation(E)[:n_neg]
        neg = torch.from_numpy(neg_np.astype(np.int32)).cuda() if n_neg else None
        y = np.zeros((B, E), dtype=np.float32)
        y[:, neg_np] = -1.0
        y[np.arange(B)[:, None], ids_np] = 1.0
        y = torch.from_numpy(y).cuda()
        fused, eager = bench_pair(lambda: K.proje_train(d, h, r, t, off, ids, off, ids, neg, LMBDA, loss),
                                  lambda: eager_step(m, h, r, t, y, y))
        labelled = 2 * (B * n_neg + B * per_row)
        print("n_neg = %3d  fused %8.1f [%.1f, %.1f]   eager %8.1f [%.1f, %.1f]   eager / fused %.2f   (%d labelled logits of %d)"
              % (n_neg, *fused, *eager, eager[0] / fused[0], labelled, 2 * B * E))


if __name__ == "__main__":
    main()
