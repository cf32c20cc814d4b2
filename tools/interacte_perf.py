#!/usr/bin/env python
"""Dev tool: the fused InteractE step (kge_interacte_train_bce) against the torch-ROCm eager restatement of the same step on the same
GPU (the torch layers in training mode as the reference writes them -- the chequer gather, the concatenated circular padding, the
grouped convolution with the repeated filter, three batch norms, three dropouts, autograd through the layers -- in front of the
existing fused head, kge_head_1n_bce through pykg2vec_amd.kernels), and the 512-query kge_interacte_eval_ranks, at two yaml presets
(FB15k: feature_permutation 1, num_filters 96, kernel_size 9; YAGO3-10: 4 / 64 / 7; both reshape 20 x 10, dropouts 0.2 / 0.5 / 0.3 of
the FB15k preset, label smoothing 0.1, B = 128, FB15k's entity and relation counts).  Warm-up, then the median, minimum and maximum of 7
rounds of 10 back-to-back calls between two events.
Usage: python tools/interacte_perf.py > profiles/r15_interacte_perf.txt"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.projection import InteractE  # noqa: E402

E, R, RH, RW, B, NQ = 14951, 1345, 20, 10, 128, 512
DROP = (0.2, 0.5, 0.3)     # input, feature map, hidden
PRESETS = {"fb15k": (1, 96, 9), "yago3_10": (4, 64, 7)}


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


def circular(x, pad):
    x = torch.cat([x[..., -pad:, :], x, x[..., :pad, :]], dim=2)
    return torch.cat([x[..., -pad:], x, x[..., :pad]], dim=3)


def eager_step(m, perm, h, r, t, off, ids, loss, g_ent, g_b):
    """torch layers (the model's own holder modules, in training mode) + the fused head with its loss and backward per direction."""
    F = torch.nn.functional
    P, ks = int(m.feature_permutation), int(m.kernel_size)
    for p in m.parameters():
        p.grad = None
    g_ent.zero_()
    g_b.zero_()
    for e in (h, t):
        comb = torch.cat([m.ent_embeddings(e), m.rel_embeddings(r)], dim=-1)
        x = comb[:, perm].reshape(-1, P, 2 * RW, RH)
        x = circular(F.dropout(m.bn0(x), DROP[0]), ks // 2)
        x = F.conv2d(x, m.conv_filt.repeat(P, 1, 1, 1), padding=0, groups=P)
        x = F.dropout2d(torch.relu(m.bn1(x)), DROP[1]).view(-1, m.flat_sz)
        x = torch.relu(m.bn2(F.dropout(m.fc(x), DROP[2])))
        dx = K.head_1n_bce(x.detach().contiguous(), m.ent_embeddings.weight.detach(), m.bias.detach(), off, ids, 0.1, loss, g_ent, g_b)
        x.backward(dx)


def run(name, P, NF, ks, rng):
    print("# %s preset: feature_permutation %d, num_filters %d, kernel_size %d (F = %d)" % (name, P, NF, ks, P * NF * 2 * RH * RW))
    m = InteractE(tot_entity=E, tot_relation=R, hidden_size=RH * RW, input_dropout=DROP[0], feature_map_dropout=DROP[1], hidden_dropout=DROP[2],
                  feature_permutation=P, num_filters=NF, kernel_size=ks, reshape_height=RH, reshape_width=RW).cuda()
    m.train()
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=1, offset=0)
    h, r, t = (torch.from_numpy(rng.integers(n, size=B)).cuda() for n in (E, R, E))
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * 4
    ids = torch.from_numpy(rng.integers(E, size=4 * B).astype(np.int32)).cuda()
    loss = K.new_loss_buffer(ws[0].device)
    fused = bench(lambda: K.interacte_train_bce(d, h, r, t, off, ids, off, ids, 0.1, loss))
    x = torch.randn(B, RH * RW, device="cuda")
    head = bench(lambda: K.head_1n_bce(x, ws[2].detach(), ws[0].detach(), off, ids, 0.1, loss, gs[2], gs[0]))
    perm = m.chequer_perm.cuda()
    eager = bench(lambda: eager_step(m, perm, h, r, t, off, ids, loss, gs[2], gs[0]))
    body = fused[0] - 2 * head[0]
    print("step   fused %9.1f [%.1f, %.1f]   eager %9.1f [%.1f, %.1f]   eager / fused %.2f   body share %.0f %% (%.1f us; the two head calls "
          "%.1f us)" % (*fused, *eager, eager[0] / fused[0], 100 * body / fused[0], body, 2 * head[0]))
    print("acceptance (fused median below eager minimum): %s" % (fused[0] < eager[1]))
    m.eval()
    trip = torch.stack([torch.from_numpy(rng.integers(n, size=NQ)) for n in (E, R, E)], 1).cuda().contiguous()
    known = torch.cat([trip, torch.stack([torch.from_numpy(rng.integers(n, size=20000)) for n in (E, R, E)], 1).cuda()])
    csrs = K.filter_csr_build(known, trip, E, R)
    de = m.make_desc(train=False)
    ranks = bench(lambda: K.interacte_eval_ranks(de, trip, *csrs))
    print("eval_ranks, %d queries   %9.1f [%.1f, %.1f]" % (NQ, *ranks))


def main():
    rng = np.random.default_rng(0)
    print("# fused InteractE step vs eager torch layers + fused head, E = %d, R = %d, reshape %d x %d, B = %d, dropouts %s; microseconds: "
          "median [min, max]" % (E, R, RH, RW, B, DROP))
    for name in sys.argv[1:] or list(PRESETS):
        run(name, *PRESETS[name], rng)


if __name__ == "__main__":
    main()
