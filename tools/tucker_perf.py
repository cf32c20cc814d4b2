#!/usr/bin/env python
"""Dev tool: the fused TuckER step (kge_tucker_train_bce) against the torch-ROCm eager restatement of the same step on the same GPU
(ATen: it forms M [2B, d1, d1] and the [B, E] tensors), at the yaml preset (d1 = d2 = 200, B = 128, FB15k shape) and at B = 4 096.
Warm-up, then the median of timed rounds of back-to-back steps between two events; the body's share is the step minus the two head
calls timed alone.  Usage: python tools/tucker_perf.py > profiles/r10_tucker_perf.txt"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.projection import TuckER  # noqa: E402

E, R, D = 14951, 1345, 200
DROP = (0.3, 0.4, 0.5)


def bench(fn, warm=5, rounds=7, inner=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner * 1e3)
    return statistics.median(out), min(out), max(out)


def eager_step(m, h, r, t, y1, y2):
    ent, rel, W = m.trainable_tensors()
    for p in (ent, rel, W):
        p.grad = None

    def fwd(e):
        a = torch.nn.functional.dropout(torch.nn.functional.normalize(ent[e], p=2, dim=1), DROP[0]).view(-1, 1, D)
        M = torch.nn.functional.dropout(torch.matmul(rel[r], W.view(D, -1)).view(-1, D, D), DROP[1])
        x = torch.nn.functional.dropout(torch.nn.functional.normalize(torch.matmul(a, M).view(-1, D), p=2, dim=1), DROP[2])
        return torch.sigmoid(torch.matmul(x, ent.T))
    bce = torch.nn.BCEWithLogitsLoss()
    (bce(fwd(t), y2) + bce(fwd(h), y1)).backward()


def main():
    rng = np.random.default_rng(0)
    print("# fused TuckER step vs eager ATen, E = %d, R = %d, d1 = d2 = %d, dropouts %s; microseconds per step: median [min, max]" % (E, R, D, DROP))
    for B in (128, 4096):
        m = TuckER(tot_entity=E, tot_relation=R, ent_hidden_size=D, rel_hidden_size=D, lmbda=0.0, input_dropout=DROP[0],
                   hidden_dropout1=DROP[1], hidden_dropout2=DROP[2]).cuda()
        ws = m.trainable_tensors()
        gs = [torch.zeros_like(w) for w in ws]
        d = m.make_desc(ws, gs, train=True, seed=1, offset=0)
        h, r, t = (torch.from_numpy(rng.integers(n, size=B)).cuda() for n in (E, R, E))
        off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * 4
        ids = torch.from_numpy(rng.integers(E, size=4 * B).astype(np.int32)).cuda()
        loss = K.new_loss_buffer(ws[0].device)
        fused = bench(lambda: K.tucker_train_bce(d, h, r, t, off, ids, off, ids, 0.1, loss))
        x = torch.randn(B, D, device="cuda")
        head = bench(lambda: K.head_1n_bce(x, ws[0].detach(), None, off, ids, 0.1, loss, gs[0]))
        y = torch.zeros(B, E, device="cuda")
        eager = bench(lambda: eager_step(m, h, r, t, y, y), rounds=5, inner=3)
        body = fused[0] - 2 * head[0]
        flops = 4 * 2.0 * (2 * B) * D * D * D     # forward tiles, g_W, g_rel, g_a tiles
        print("B = %5d  fused %9.1f [%.1f, %.1f]   eager %9.1f [%.1f, %.1f]   ratio %.2f   body share %.0f %% (%.1f us: %.2f TFLOP/s on the"
              " matrix cores, %.0f GB/s effective on W at 4 passes)" % (B, *fused, *eager, eager[0] / fused[0], 100 * body / fused[0], body,
                                                                        flops / body / 1e6, 4 * D * D * D * 4 / body / 1e3))


if __name__ == "__main__":
    main()
