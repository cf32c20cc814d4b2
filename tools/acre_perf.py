#!/usr/bin/env python
"""Dev tool: the fused AcrE step (kge_acre_train_bce, the serial way or with --way parallel the parallel way) against the torch-ROCm eager restatement of the same step on the same
GPU (the torch layers in training mode as the reference writes them -- bn0, input dropout, the three dilated convolutions and the residual (parallel: the three
convolutions of the input and the shared 1600 -> 400 gate), bn1, relu, Dropout2d, fc, hidden dropout, bn2, relu, autograd through the layers -- in front of the existing fused head,
kge_head_1n_bce through pykg2vec_amd.kernels), and the 512-query kge_acre_eval_ranks, at the FB15k preset (in_channels 32, dilations
1 / 2 / 2, acre_bias, dropouts 0.2 / 0.2 / 0.2, label smoothing 0.1, FB15k's entity and relation counts) for one batch size.  Warm-up,
then the median, minimum and maximum of 7 rounds of 10 back-to-back calls between two events.
Usage: python tools/acre_perf.py [--way serial|parallel] [--fused-only] 128 >> profiles/r16_acre_perf.txt; python tools/acre_perf.py 256
>> ... (one process per batch size; run each under its own time limit).  --fused-only times the fused step and the rank pass alone,
for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/acre_perf.py --way parallel --fused-only 128) that holds no
eager kernels."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402
from pykg2vec_amd.projection import AcrE  # noqa: E402

E, R, C, NQ = 14951, 1345, 32, 512
DIL = (1, 2, 2)
DROP = (0.2, 0.2, 0.2)     # input, feature map, hidden


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


def eager_step(m, h, r, t, off, ids, loss, g_ent, g_b, way="serial"):
    """torch layers (the model's own holder modules, in training mode) + the fused head with its loss and backward per direction."""
    F = torch.nn.functional
    for p in m.parameters():
        p.grad = None
    g_ent.zero_()
    g_b.zero_()
    for e in (h, t):
        x = torch.cat([m.ent_embeddings(e).view(-1, 1, 10, 20), m.rel_embeddings(r).view(-1, 1, 10, 20)], dim=2)
        x = F.dropout(m.bn0(x), DROP[0])
        if way == "serial":
            x = m.conv3(m.conv2(m.conv1(x))) + x
        else:
            g_in = torch.cat([x.expand(-1, C, 20, 20).reshape(-1, C, 400)] + [conv(x).view(-1, C, 400) for conv in (m.conv1, m.conv2, m.conv3)], 2)
            x = m.W_gate_e(g_in).view(-1, C, 20, 20)
        x = F.dropout2d(torch.relu(m.bn1(x)), DROP[1]).view(x.shape[0], -1)
        x = torch.relu(m.bn2(F.dropout(m.fc(x), DROP[2])))
        dx = K.head_1n_bce(x.detach().contiguous(), m.ent_embeddings.weight.detach(), m.bias.detach(), off, ids, 0.1, loss, g_ent, g_b)
        x.backward(dx)


def run(B, rng, way="serial", fused_only=False):
    m = AcrE(tot_entity=E, tot_relation=R, hidden_size=200, input_dropout=DROP[0], feature_map_dropout=DROP[1], hidden_dropout=DROP[2],
             in_channels=C, way=way, first_atrous=DIL[0], second_atrous=DIL[1], third_atrous=DIL[2], acre_bias=True).cuda()
    m.train()
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=1, offset=0)
    h, r, t = (torch.from_numpy(rng.integers(n, size=B)).cuda() for n in (E, R, E))
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * 4
    ids = torch.from_numpy(rng.integers(E, size=4 * B).astype(np.int32)).cuda()
    loss = K.new_loss_buffer(ws[0].device)
    fused = bench(lambda: K.acre_train_bce(d, h, r, t, off, ids, off, ids, 0.1, loss))
    if fused_only:
        print("B = %d   step   fused %9.1f [%.1f, %.1f]" % (B, *fused))
    if not fused_only:
        x = torch.randn(B, 200, device="cuda")
        head = bench(lambda: K.head_1n_bce(x, ws[1].detach(), ws[0].detach(), off, ids, 0.1, loss, gs[1], gs[0]))
        eager = bench(lambda: eager_step(m, h, r, t, off, ids, loss, gs[1], gs[0], way))
        body = fused[0] - 2 * head[0]
        print("B = %d   step   fused %9.1f [%.1f, %.1f]   eager %9.1f [%.1f, %.1f]   eager / fused %.2f   body share %.0f %% (%.1f us; the two "
              "head calls %.1f us)" % (B, *fused, *eager, eager[0] / fused[0], 100 * body / fused[0], body, 2 * head[0]))
        print("B = %d   fused median below eager minimum: %s" % (B, fused[0] < eager[1]))
    m.eval()
    trip = torch.stack([torch.from_numpy(rng.integers(n, size=NQ)) for n in (E, R, E)], 1).cuda().contiguous()
    known = torch.cat([trip, torch.stack([torch.from_numpy(rng.integers(n, size=20000)) for n in (E, R, E)], 1).cuda()])
    csrs = K.filter_csr_build(known, trip, E, R)
    de = m.make_desc(train=False)
    ranks = bench(lambda: K.acre_eval_ranks(de, trip, *csrs))
    print("B = %d   eval_ranks, %d queries   %9.1f [%.1f, %.1f]" % (B, NQ, *ranks))


def main():
    rng = np.random.default_rng(0)
    args = sys.argv[1:]
    way = "serial"
    if "--way" in args:
        way = args[args.index("--way") + 1]
        del args[args.index("--way"):args.index("--way") + 2]
    assert way in ("serial", "parallel"), way
    fused_only = "--fused-only" in args
    args = [a for a in args if a != "--fused-only"]
    print("# fused AcrE step (%s, in_channels %d, dilations %s) vs eager torch layers + fused head, E = %d, R = %d, dropouts %s; "
          "microseconds: median [min, max]" % (way, C, DIL, E, R, DROP))
    for B in [int(a) for a in args] or [128]:
        run(B, rng, way, fused_only)


if __name__ == "__main__":
    main()
