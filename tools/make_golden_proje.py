#!/usr/bin/env python
"""Freeze the LIVE reference's ProjE_pointwise outputs into tests/golden/ref_proje{,_neg}.npz (build container only: the reference tree
is imported through oracle/ref_shim.py), run in float64 on tables that are exact in fp32.  hidden_dropout 0 (torch's masks cannot be
reproduced), E = 70, R = 5, k = 20, B = 9, lmbda = 0.01, the xavier tables scaled by 4 (logits of a few units, far from both clamps).

Recorded: the eight tables, the batch ids, the dense label rows (training split only) and the negative list, the losses of both
directions (ProjE_pointwise.forward), the regulariser (get_reg), their total (utils/trainer.py:169-172), the eight autograd gradients,
and the [4, n] ranks of a small test split as the reference's MetricCalculator counts them (utils/evaluator.py:70-123 on
predict_tail_rank / predict_head_rank).  Every recorded rank is recomputed in float64 (tools/proje_reference.py) and must equal the
recorded one, with no other candidate within MIN_GAP of the true entity's prediction: that is what entitles the GPU test to demand
exact ranks.  Fixed seeds: a second run writes identical arrays.

  ref_proje       positives only (neg_rate 0)
  ref_proje_neg   positives plus a recorded list of 70 negative ids -- np.random.permutation(E)[0:100] at E = 70 -- written as -1 into
                  every row and both directions except on the row's positives (data/generator.py:200-239)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
import torch  # noqa: E402
from pykg2vec.models.projection import ProjE_pointwise  # noqa: E402
from tools import proje_reference as pr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
E, R, K, B, N_TRAIN, N_TEST, LMBDA, SCALE = 70, 5, 20, 9, 120, 12, 0.01, 4.0
MIN_GAP = 1e-6
CASES = {"proje": (False, 7201), "proje_neg": (True, 7202)}


def scan(cand, true, known):
    """get_tail_rank / get_head_rank: walk the candidates from the end until the true entity shows up."""
    rank = frank = 0
    for j in range(len(cand)):
        v = int(cand[-j - 1])
        if v == true:
            break
        rank += 1
        frank += 0 if v in known else 1
    return rank, frank


def golden(name, negatives, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    model = ProjE_pointwise(tot_entity=E, tot_relation=R, hidden_size=K, lmbda=LMBDA, hidden_dropout=0.0, device="cpu")
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(SCALE)
    model.double()   # the reference's own code in float64 on fp32-representable tables: the fixture carries no fp32 rounding of its own
    trip = np.unique(np.stack([rng.integers(E, size=400), rng.integers(R, size=400), rng.integers(E, size=400)], 1), axis=0)
    trip = trip[rng.permutation(len(trip))]
    train, test = trip[:N_TRAIN], trip[N_TRAIN:N_TRAIN + N_TEST]
    valid = trip[N_TRAIN + N_TEST:N_TRAIN + 2 * N_TEST]
    known = np.concatenate([train, valid, test])
    h, r, t = (torch.from_numpy(np.ascontiguousarray(train[:B, k])) for k in range(3))
    neg = rng.permutation(E)[0:100] if negatives else np.zeros(0, dtype=np.int64)
    hr_t, tr_h = np.zeros((B, E), np.float64), np.zeros((B, E), np.float64)
    for i, (a, b, c) in enumerate(train[:B]):
        tails, heads = train[(train[:, 0] == a) & (train[:, 1] == b), 2], train[(train[:, 2] == c) & (train[:, 1] == b), 0]
        hr_t[i, tails] = 1.0
        tr_h[i, heads] = 1.0
        for idx in neg:   # data/generator.py:211-217
            if idx not in tails:
                hr_t[i, idx] += -1.0
            if idx not in heads:
                tr_h[i, idx] += -1.0
    model.train()
    loss_tail = model(h, r, torch.from_numpy(hr_t), direction="tail")
    loss_head = model(t, r, torch.from_numpy(tr_h), direction="head")
    reg = model.get_reg(h, r, t)
    loss = model.loss(loss_head, loss_tail) + reg
    loss.backward()
    rec = {"E": E, "R": R, "k": K, "lmbda": LMBDA, "train": train, "valid": valid, "test": test, "h": h.numpy(), "r": r.numpy(),
           "t": t.numpy(), "hr_t": hr_t, "tr_h": tr_h, "neg": neg.astype(np.int64), "loss_tail": np.float64(loss_tail.item()),
           "loss_head": np.float64(loss_head.item()), "reg": np.float64(reg.item()), "loss": np.float64(loss.item())}
    for k, v in model.state_dict().items():
        rec[k] = v.detach().numpy().copy()
    for k, p in model.named_parameters():
        rec["grad." + k] = p.grad.numpy().copy()
    model.eval()
    got = np.zeros((4, len(test)), dtype=np.int64)
    with torch.no_grad():
        for i, (a, b, c) in enumerate(test):
            a, b, c = int(a), int(b), int(c)
            tails = model.predict_tail_rank(torch.LongTensor([a]), torch.LongTensor([b]), topk=E).view(-1).numpy()
            heads = model.predict_head_rank(torch.LongTensor([c]), torch.LongTensor([b]), topk=E).view(-1).numpy()
            got[1, i], got[3, i] = scan(tails, c, set(known[(known[:, 0] == a) & (known[:, 1] == b), 2].tolist()))
            got[0, i], got[2, i] = scan(heads, a, set(known[(known[:, 2] == c) & (known[:, 1] == b), 0].tolist()))
    rec["ranks"] = got
    P = {k: rec[k].astype(np.float64) for k in pr.TABLES}
    want, gap = pr.ranks(P, test, known)
    if not gap > MIN_GAP:
        raise SystemExit("%s: a competitor lies %.3g from a true candidate (<= %g): pick another seed" % (name, gap, MIN_GAP))
    if not np.array_equal(want, got):
        raise SystemExit("%s: float64 ranks differ from the reference's:\n%s\n%s" % (name, want, got))
    path = os.path.join(OUT, "ref_%s.npz" % name)
    np.savez_compressed(path, **rec)
    st = pr.step(P, rec["h"], rec["r"], rec["t"], hr_t, tr_h, LMBDA)
    zmax = max(np.abs(st["logits_tail"]).max(), np.abs(st["logits_head"]).max())
    print("wrote %s: loss %.9f (tail %.6f, head %.6f, reg %.6f), largest |logit| %.3g, smallest neighbour gap %.3g, %d bytes"
          % (name, rec["loss"], rec["loss_tail"], rec["loss_head"], rec["reg"], zmax, gap, os.path.getsize(path)))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (negatives, seed) in CASES.items():
        if not only or name in only:
            golden(name, negatives, seed)
