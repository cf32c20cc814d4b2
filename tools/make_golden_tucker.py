#!/usr/bin/env python
"""Freeze the LIVE reference's TuckER outputs into tests/golden/ref_tucker{,_ls}.npz (build container only: the reference tree is
imported through oracle/ref_shim.py), run in float64 on tables that are exact in fp32.  All dropouts 0 (torch's masks cannot be reproduced), E = 70, R = 5, d1 = 20, d2 = 12, B = 9.

Recorded: the three tables, the batch ids, the dense label rows (training split only), the [B, E] predictions of both directions, the
loss of Criterion.multi_class_bce, the three autograd gradients, and the [4, n] ranks of a small test split as the reference's
MetricCalculator counts them (utils/evaluator.py:70-123 on predict_tail_rank / predict_head_rank).  Every recorded rank is recomputed in
float64 (tools/tucker_reference.py) and must equal the recorded one, with no other candidate within MIN_GAP of the true entity's
prediction: that is what entitles the GPU test to demand exact ranks.  Fixed seeds: a second run writes identical arrays.

  ref_tucker      no label smoothing
  ref_tucker_ls   label smoothing 0.1
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
from pykg2vec.models.projection import TuckER  # noqa: E402
from pykg2vec.utils.criterion import Criterion  # noqa: E402
from tools import tucker_reference as tr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
E, R, D1, D2, B, N_TRAIN, N_TEST = 70, 5, 20, 12, 9, 120, 12
MIN_GAP = 1e-6
CASES = {"tucker": (None, 7101), "tucker_ls": (0.1, 7102)}


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


def golden(name, ls, seed):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    model = TuckER(tot_entity=E, tot_relation=R, ent_hidden_size=D1, rel_hidden_size=D2, lmbda=0.0, input_dropout=0.0,
                   hidden_dropout1=0.0, hidden_dropout2=0.0)
    with torch.no_grad():   # xavier tables of this size give predictions within 1e-3 of 0.5: spread them
        for p in model.parameters():
            p.mul_(6.0)
    model.double()   # the reference's own code in float64 on fp32-representable tables: the fixture carries no fp32 rounding of its own
    trip = np.unique(np.stack([rng.integers(E, size=400), rng.integers(R, size=400), rng.integers(E, size=400)], 1), axis=0)
    trip = trip[rng.permutation(len(trip))]
    train, test = trip[:N_TRAIN], trip[N_TRAIN:N_TRAIN + N_TEST]
    valid = trip[N_TRAIN + N_TEST:N_TRAIN + 2 * N_TEST]
    known = np.concatenate([train, valid, test])
    h, r, t = (torch.from_numpy(np.ascontiguousarray(train[:B, k])) for k in range(3))
    hr_t, tr_h = np.zeros((B, E), np.float64), np.zeros((B, E), np.float64)
    for i, (a, b, c) in enumerate(train[:B]):
        hr_t[i, train[(train[:, 0] == a) & (train[:, 1] == b), 2]] = 1.0
        tr_h[i, train[(train[:, 2] == c) & (train[:, 1] == b), 0]] = 1.0
    model.train()
    pred_tails, pred_heads = model(h, r, direction="tail"), model(t, r, direction="head")
    loss = Criterion.multi_class_bce(pred_heads, pred_tails, torch.from_numpy(tr_h), torch.from_numpy(hr_t), ls, E if ls is not None else None)
    loss.backward()
    rec = {"E": E, "R": R, "d1": D1, "d2": D2, "label_smoothing": -1.0 if ls is None else ls, "train": train, "valid": valid, "test": test,
           "h": h.numpy(), "r": r.numpy(), "t": t.numpy(), "hr_t": hr_t, "tr_h": tr_h, "pred_tails": pred_tails.detach().numpy(),
           "pred_heads": pred_heads.detach().numpy(), "loss": np.float64(loss.item())}
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
    P = {k: rec[k].astype(np.float64) for k in ("ent_embeddings.weight", "rel_embeddings.weight", "W.weight")}
    want, gap = tr.ranks(P, test, known)
    if not gap > MIN_GAP:
        raise SystemExit("%s: a competitor lies %.3g from a true candidate (<= %g): pick another seed" % (name, gap, MIN_GAP))
    if not np.array_equal(want, got):
        raise SystemExit("%s: float64 ranks differ from the reference's:\n%s\n%s" % (name, want, got))
    path = os.path.join(OUT, "ref_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote %s: loss %.9f, smallest neighbour gap %.3g, %d bytes" % (name, rec["loss"], gap, os.path.getsize(path)))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, (ls, seed) in CASES.items():
        if not only or name in only:
            golden(name, ls, seed)
