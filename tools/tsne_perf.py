#!/usr/bin/env python
"""Dev tool: the t-SNE projection (csrc/kge_tsne.hip) at FB15k's shape (E = 14 951, d = 100, float32 normal rows from a seed),
perplexity 30, 1 000 iterations.  Set-up (search + affinities + joint) and the descent are timed apart: a warm-up, then the median
[min, max] of 7 rounds between two events.  The descent is compared with a plain-torch composition of the SAME iteration on the same
card (the dense [n, n] w block in row chunks, the attraction through index_add over the CSR entries); the baseline is not the code
under test.  If sklearn imports, one TSNE(method="barnes_hut") run on the CPU is reported as what it is: a different algorithm on a
different device, a wall-clock for orientation and no ratio to claim.
Usage: python tools/tsne_perf.py > profiles/r27_tsne_perf.txt
       python tools/tsne_perf.py --trace     (set-up once and 20 iterations: for one separate kernel trace)
       python tools/tsne_perf.py --no-sklearn"""
import os
import statistics
import sys
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402

E, D, PERPLEXITY, ITERS, EXAG_ITERS = 14951, 100, 30.0, 1000, 250
KNN = int(3 * PERPLEXITY)
LR = max(E / 12.0 / 4.0, 50.0)


def timed(fn, warm=1, rounds=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def setup(table):
    own = torch.arange(E, dtype=torch.int64, device=table.device)
    ids, dist, count = K.knn_rows(table, table, KNN, metric="l2", self_ids=own)
    cond_p, _ = K.tsne_affinities(ids, dist, count, PERPLEXITY)
    return K.tsne_joint(ids, cond_p, count)


def descent(csr, Y0, iters=ITERS, stop=EXAG_ITERS):
    Y = Y0.clone()
    update, gains = K.tsne_state(Y)
    K.tsne_run(csr, Y, min(stop, iters), it0=0, exaggeration=12.0, momentum=0.5, learning_rate=LR, update=update, gains=gains)
    K.tsne_run(csr, Y, iters - min(stop, iters), it0=min(stop, iters), exaggeration=1.0, momentum=0.8, learning_rate=LR, update=update, gains=gains)
    return Y


def torch_iteration(csr, rows, Y, update, gains, exaggeration, momentum, chunk=2048):
    """One iteration of the same step in torch ops: w in [chunk, n] blocks, the attraction over the CSR entries."""
    n = Y.shape[0]
    rep = torch.empty_like(Y)
    Z = torch.zeros((), dtype=torch.float64, device=Y.device)
    for a in range(0, n, chunk):
        d = Y[a:a + chunk, None, :] - Y[None, :, :]
        w = 1.0 / (1.0 + (d * d).sum(-1))
        w[torch.arange(w.shape[0], device=Y.device), torch.arange(a, a + w.shape[0], device=Y.device)] = 0
        Z += w.sum(dtype=torch.float64)
        rep[a:a + chunk] = ((w * w)[:, :, None] * d).sum(1)
    dj = Y[rows] - Y[csr.col.long()]
    pw = csr.val * exaggeration / (1.0 + (dj * dj).sum(-1))
    attr = torch.zeros_like(Y).index_add_(0, rows, pw[:, None] * dj)
    grad = 4.0 * (attr - rep / Z.float())
    inc = update * grad < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    update.mul_(momentum).sub_(LR * gains * grad)
    Y.add_(update)


def torch_descent(csr, Y0, iters):
    Y = Y0.clone()
    update, gains = torch.zeros_like(Y), torch.ones_like(Y)
    rows = torch.repeat_interleave(torch.arange(csr.n, device=Y.device), csr.row_off[1:] - csr.row_off[:-1])
    for it in range(iters):
        torch_iteration(csr, rows, Y, update, gains, 12.0 if it < EXAG_ITERS else 1.0, 0.5 if it < EXAG_ITERS else 0.8)
    return Y


rng = np.random.default_rng(27)
table = torch.from_numpy(rng.normal(size=(E, D)).astype(np.float32)).cuda()
gen = torch.Generator(device="cpu")
gen.manual_seed(0)
Y0 = (1e-4 * torch.randn((E, 2), generator=gen)).cuda()

if "--trace" in sys.argv:
    csr = setup(table)
    descent(csr, Y0, iters=20, stop=10)
    torch.cuda.synchronize()
    sys.exit(0)

print("command: python tools/tsne_perf.py   (E = %d, d = %d, float32 normal rows, perplexity %g: %d neighbours, %d iterations of "
      "which %d exaggerated, learning rate %.1f; %s)" % (E, D, PERPLEXITY, KNN, ITERS, EXAG_ITERS, LR, torch.cuda.get_device_name(0)))
t_setup = timed(lambda: setup(table))
csr = setup(table)
print("set-up (knn_rows l2 k = %d + tsne_affinities + tsne_joint, nnz = %d): %.2f [%.2f, %.2f] ms" % (KNN, csr.nnz, *t_setup))
t_run = timed(lambda: descent(csr, Y0))
per_it = t_run[0] / ITERS * 1e3
print("descent, %d iterations in two kge_tsne_run calls: %.1f [%.1f, %.1f] ms = %.1f us per iteration" % (ITERS, *t_run, per_it))
# the sweep's share of its VALU bound, counted from the shape: per pair 2 subtractions, 2 FMAs, 1 reciprocal at quarter rate (4 issue
# slots), 1 add, 1 multiply, 2 FMAs = 12 slots; 256 CUs x 4 SIMDs x 16 lanes per clock
pairs = float(E) * float(E)
clock = 2.4e9
bound_us = pairs * 12 / (256 * 4 * 16 * clock) * 1e6
print("repulsion sweep: %.0f M pairs x 12 VALU issue slots = %.1f us per iteration at %.1f GHz on 256 CUs (the kernel's own time: the "
      "separate kernel trace; the whole iteration above is %.2f x this bound)" % (pairs / 1e6, bound_us, clock / 1e9, per_it / bound_us))
base_iters = 20
t_base = timed(lambda: torch_descent(csr, Y0, base_iters), rounds=3)
base_it = t_base[0] / base_iters * 1e3
print("the same iteration in torch ops ([2048, n] w blocks + index_add), %d iterations: %.1f [%.1f, %.1f] ms = %.1f us per iteration; "
      "ratio %.1f (%s)" % (base_iters, *t_base, base_it, base_it / per_it,
                           "kge_tsne_run FASTER than the torch composition" if base_it > per_it else "kge_tsne_run SLOWER than the torch composition"))
# both run the same map for a few iterations: the gradient is the same function
a, b = descent(csr, Y0, iters=5, stop=5), torch_descent(csr, Y0, 5)
print("after 5 iterations from the same init: max |Y - Y_torch| = %.3g of max |Y| = %.3g" % ((a - b).abs().max().item(), b.abs().max().item()))
if "--no-sklearn" not in sys.argv:
    try:
        from sklearn.manifold import TSNE
    except Exception as e:  # noqa: BLE001
        print("sklearn: not importable here (%s): no CPU wall-clock" % type(e).__name__)
    else:
        t0 = time.time()
        kw = dict(n_components=2, perplexity=PERPLEXITY, method="barnes_hut", init="random", random_state=0, n_jobs=16)
        try:
            TSNE(max_iter=ITERS, **kw).fit_transform(table.cpu().numpy())
        except TypeError:
            TSNE(n_iter=ITERS, **kw).fit_transform(table.cpu().numpy())
        print("sklearn TSNE(method=\"barnes_hut\", %d iterations, n_jobs=16) on the CPU: %.1f s wall-clock -- a different algorithm "
              "(approximate repulsion, early stopping) on a different device: orientation, not a ratio to claim" % (ITERS, time.time() - t0))
