#!/usr/bin/env python
"""Dev tool: PCA (csrc/kge_pca.hip) at FB15k's entity count (E = 14 951; d = 100, 400 and 512; float32 rows with a geometric spectrum
around a random mean): the fused pair K.pca_fit + K.pca_transform to 2 components against the torch composition inside
Evaluator._projection_init -- float64 centring, Xc^T Xc, torch.linalg.eigh, the sign rule, Xc @ top -- which is the baseline and not
the code under test.  Warm-up, then the median [min, max] of 5 rounds of 2 back-to-back calls between two events, the rounds of the two
paths alternating.  A fused call includes its workspace and output allocations.  Peak device memory: the fused call's workspace
(kge_pca_workspace_bytes) and outputs against torch's peak allocation during the composition.  The Jacobi solver runs in ONE workgroup
by choice (no grid-wide barrier on a shared card): where the composition is faster the line says so.  The card is shared: times move
from run to run; the ratio of alternating rounds is the steadier figure.
Usage: python tools/pca_perf.py > profiles/r35_pca_perf.txt"""
import os
import statistics
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pykg2vec_amd import kernels as K  # noqa: E402


def bench(fns, warm=1, rounds=5, inner=2):
    """One (median, min, max) in us per call for every function: the rounds of the functions alternate, so that a drift of the
    machine falls on all of them; a round is `inner` back-to-back calls between two events."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for fn, times in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / inner * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in out]


def composed(X):
    """The PCA lines of Evaluator._projection_init, without its final scaling: -> Y float64 [n, 2], eigenvalues ascending."""
    Xc = X.double() - X.double().mean(0, keepdim=True)
    lam, vec = torch.linalg.eigh(Xc.t() @ Xc / max(X.shape[0] - 1, 1))
    top = vec[:, -2:].flip(1)
    big = top.gather(0, top.abs().argmax(0, keepdim=True))
    top = top * torch.where(big < 0, -torch.ones_like(big), torch.ones_like(big))
    return Xc @ top, lam


def fused(X):
    fit = K.pca_fit(X)
    return K.pca_transform(X, fit, 2), fit


E = 14951
print("command: python tools/pca_perf.py   (E = %d; %s; a shared card)" % (E, torch.cuda.get_device_name(0)))
for D in (100, 400, 512):
    rng = np.random.default_rng(D)
    X = torch.from_numpy((rng.normal(size=(E, D)) * 0.97 ** np.arange(D) + rng.normal(size=D)).astype(np.float32)).cuda()
    t_fused, t_base = bench([lambda: fused(X), lambda: composed(X)])
    (Y, fit), (_, again) = fused(X), fused(X)
    t_fit, t_tr = bench([lambda: K.pca_fit(X), lambda: K.pca_transform(X, fit, 2)], rounds=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    Yb, lam = composed(X)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    ws = K.pca_workspace_bytes(E, D)
    ratio = t_base[0] / t_fused[0]
    print("d = %3d: fit + transform %10.1f [%.1f, %.1f] us (fit %.1f, transform %.1f), %d Jacobi sweeps   torch composition %10.1f [%.1f, %.1f] us   "
          "ratio %.2f (%s)   max |eigenvalue - eigh| / largest %.2e, max |Y - composition| / max |Y| %.2e, results repeat: %s   "
          "device memory: fused %.2f MB (workspace %.2f MB), composition peak %.1f MB"
          % (D, *t_fused, t_fit[0], t_tr[0], int(fit.sweeps.item()), *t_base, ratio, "fused FASTER" if ratio > 1 else "fused SLOWER",
             float((fit.explained_variance - lam.flip(0)).abs().max() / lam.max()), float((Y.double() - Yb).abs().max() / Yb.abs().max()),
             all(torch.equal(getattr(fit, f), getattr(again, f)) for f in fit._fields),
             (ws + 16 * D * D + 16 * D + 8 + 8 * E) / 1e6, ws / 1e6, peak / 1e6))
torch.cuda.synchronize()
