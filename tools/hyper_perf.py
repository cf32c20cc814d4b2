#!/usr/bin/env python
"""Dev tool: the fused HypER step (kge_hyper_train_bce) against the torch-ROCm eager restatement of the same step on the same GPU (the
torch layers in training mode as the reference writes them -- fc1, the grouped convolution with its permutes, three batch norms, three
dropouts, autograd through the layers -- in front of the existing fused head, kge_head_1n_bce through pykg2vec_amd.kernels), and the
512-query kge_hyper_eval_ranks, at the yaml preset (ent_hidden_size 200, rel_hidden_size 200, dropouts 0.2 / 0.2 / 0.3, label smoothing
0.1, B = 128, FB15k shape).  Warm-up, then the median, minimum and maximum of 7 rounds of 10 back-to-back calls between two events.
Usage: python tools/hyper_perf.py > profiles/r14_hyper_perf.txt"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.projection import HypER  # noqa: E402

E, R, D, DR, B, NQ = 14951, 1345, 200, 200, 128, 512
DROP = (0.2, 0.2, 0.3)


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


def eager_step(m, h, r, t, off, ids, loss, g_ent, g_b):
    """torch layers (the model's own holder modules, in training mode) + the fused head with its loss and backward per direction."""
    F = torch.nn.functional
    for p in m.parameters():
        p.grad = None
    g_ent.zero_()
    g_b.zero_()
    for e in (h, t):
        n = e.numel()
        x = F.dropout(m.bn0(m.ent_embeddings(e).view(-1, 1, 1, D)), DROP[0])
        k = m.fc1(m.rel_embeddings(r)).view(n * 32, 1, 1, 9)
        x = F.conv2d(x.permute(1, 0, 2, 3), k, groups=n).view(n, 1, 32, 1, D - 8)
        x = torch.sum(x.permute(0, 3, 4, 1, 2), dim=3).permute(0, 3, 1, 2).contiguous()
        x = F.dropout2d(m.bn1(x), DROP[1]).view(n, -1)
        x = torch.relu(m.bn2(F.dropout(m.fc(x), DROP[2])))
        dx = K.head_1n_bce(x.detach().contiguous(), m.ent_embeddings.weight.detach(), m.b.detach(), off, ids, 0.1, loss, g_ent, g_b)
        x.backward(dx)


def main():
    rng = np.random.default_rng(0)
    print("# fused HypER step vs eager torch layers + fused head, E = %d, R = %d, hidden sizes %d / %d, B = %d, dropouts %s; microseconds: "
          "median [min, max]" % (E, R, D, DR, B, DROP))
    m = HypER(tot_entity=E, tot_relation=R, ent_hidden_size=D, rel_hidden_size=DR, input_dropout=DROP[0], feature_map_dropout=DROP[1],
              hidden_dropout=DROP[2]).cuda()
    m.train()
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=1, offset=0)
    h, r, t = (torch.from_numpy(rng.integers(n, size=B)).cuda() for n in (E, R, E))
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * 4
    ids = torch.from_numpy(rng.integers(E, size=4 * B).astype(np.int32)).cuda()
    loss = K.new_loss_buffer(ws[0].device)
    fused = bench(lambda: K.hyper_train_bce(d, h, r, t, off, ids, off, ids, 0.1, loss))
    x = torch.randn(B, D, device="cuda")
    head = bench(lambda: K.head_1n_bce(x, ws[1].detach(), ws[0].detach(), off, ids, 0.1, loss, gs[1], gs[0]))
    eager = bench(lambda: eager_step(m, h, r, t, off, ids, loss, gs[1], gs[0]))
    body = fused[0] - 2 * head[0]
    print("step   fused %9.1f [%.1f, %.1f]   eager %9.1f [%.1f, %.1f]   eager / fused %.2f   body share %.0f %% (%.1f us; the two head calls "
          "%.1f us)" % (*fused, *eager, eager[0] / fused[0], 100 * body / fused[0], body, 2 * head[0]))
    print("acceptance (fused median below eager minimum): %s" % (fused[0] < eager[1]))
    m.eval()
    trip = torch.stack([torch.from_numpy(rng.integers(n, size=NQ)) for n in (E, R, E)], 1).cuda().contiguous()
    known = torch.cat([trip, torch.stack([torch.from_numpy(rng.integers(n, size=20000)) for n in (E, R, E)], 1).cuda()])
    csrs = K.filter_csr_build(known, trip, E, R)
    de = m.make_desc(train=False)
    ranks = bench(lambda: K.hyper_eval_ranks(de, trip, *csrs))
    print("eval_ranks, %d queries   %9.1f [%.1f, %.1f]" % (NQ, *ranks))


if __name__ == "__main__":
    main()
