#!/usr/bin/env python
"""Freeze the LIVE reference's AcrE outputs into tests/golden/ref_acre{,_ls,_masked,_parallel,_parallel_masked}.npz (build container
only: the reference tree is imported through oracle/ref_shim.py), run in float64 on tensors that are exact in fp32.  E = 70, R = 5,
in_channels = 3 (neither a multiple of 4 nor of 16), dilations 1 / 2 / 3, B = 9, a test split of 12.

  ref_acre                  serial, acre_bias, rates 0, no label smoothing
  ref_acre_ls               serial, no acre_bias, label smoothing 0.1
  ref_acre_masked           serial, rates 0.2 / 0.2 / 0.3 (input / feature map / hidden), label smoothing 0.1: the model's three dropout
                            modules are replaced by modules that multiply by a given mask, and the masks are the Philox masks of a
                            recorded (seed, offset) (tools/acre_reference.py:masks), which are recorded too
  ref_acre_parallel         parallel, acre_bias, rates 0, label smoothing 0.1
  ref_acre_parallel_masked  parallel, the same rates under masks

The batch norm weights and biases and `bias` are randomised (nothing sits at a cancelling default), the running buffers were filled by
two training forwards on other rows, and everything is rounded to fp32.  The batch and the test split hold id 0 of both tables (no
padding_idx: its gradient is an ordinary row).  fc.weight [200, 1200] and W_gate_e.weight [400, 1600] are too large to record whole:
their VALUES are RandomState(seed).uniform(-1, 1) * scale rounded to fp32 and only (seed, scale) is recorded ("gen.<key>"); of their
GRADIENTS a fixed sample is recorded in float64 (4096 flat indices from a recorded RandomState seed, plus the arg-max entry), with each
gradient's max-abs and sum.  Recorded besides: the state dict's key list in order, the state BEFORE the step, the batch ids and dense
label rows, the eval-form predictions of both directions and the [4, n] eval-form ranks of the test split as the reference's
MetricCalculator counts them, then the training step: both prediction tensors, the loss of Criterion.multi_class_bce, the autograd
gradients, the six running buffers and the three counters after the step.  The script refuses (pick another seed) unless
tools/acre_reference.py reproduces every recorded float to 1e-10 of the array's max-abs and every rank exactly, no competitor lies
within MIN_GAP of a true candidate's prediction, no bn1 or bn2 output (both forms; each feeds a relu) is within MIN_MARGIN of zero and,
in the masked cases, every site of each direction both keeps and drops something.  Fixed seeds: a second run writes identical arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
import torch  # noqa: E402
from pykg2vec.models.projection import AcrE  # noqa: E402
from pykg2vec.utils.criterion import Criterion  # noqa: E402
from tools import acre_reference as ar  # noqa: E402
from tools.make_golden_conve import MaskDrop  # noqa: E402
from tools.make_golden_tucker import scan  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
E, R, C, A1, A2, A3, B, N_TRAIN, N_TEST = 70, 5, 3, 1, 2, 3, 9, 120, 12
K = 200
MIN_GAP, MIN_MARGIN, RTOL = 1e-6, 1e-5, 1e-10
RATES = (0.2, 0.2, 0.3)
# name: (way, acre_bias, label smoothing, dropout rates (input, feature map, hidden), seed, (mask seed, mask offset))
CASES = {"acre": ("serial", True, None, (0.0, 0.0, 0.0), 7501, None),
         "acre_ls": ("serial", False, 0.1, (0.0, 0.0, 0.0), 7502, None),
         "acre_masked": ("serial", True, 0.1, RATES, 7503, ((5 << 32) | 11, 3)),
         "acre_parallel": ("parallel", True, 0.1, (0.0, 0.0, 0.0), 7504, None),
         "acre_parallel_masked": ("parallel", True, 0.1, RATES, 7508, ((7 << 32) | 13, 2))}


def close(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, ref = np.abs(got - want).max(), np.abs(want).max()
    if not err <= RTOL * max(ref, 1e-300):
        raise SystemExit("%s: the restatement is off by %.3g (max-abs %.3g)" % (name, err, ref))


def golden(name, way, acre_bias, ls, rates, seed, mask_key):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    model = AcrE(tot_entity=E, tot_relation=R, hidden_size=K, input_dropout=rates[0], hidden_dropout=rates[2], feature_map_dropout=rates[1],
                 in_channels=C, way=way, first_atrous=A1, second_atrous=A2, third_atrous=A3, acre_bias=acre_bias)
    G = dict(in_channels=C, way=way, first_atrous=A1, second_atrous=A2, third_atrous=A3, acre_bias=acre_bias)
    shp = ar.shapes(G, E, R)
    gen = {}
    with torch.no_grad():   # nothing at a cancelling default
        for bn in (model.bn0, model.bn1, model.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        model.bias.uniform_(-0.5, 0.5)
        for i, key in enumerate(ar.LARGE):   # the large tensors: values from a recorded seed, at the scale of the reference's own init
            if key in shp:
                p = dict(model.named_parameters())[key]
                gen[key] = (seed * 10 + i, 1.0 / np.sqrt(shp[key][1]))
                p.copy_(torch.from_numpy(ar.gen_tensor(gen[key][0], gen[key][1], shp[key])))
    model.double()   # the reference's own code in float64 on fp32-representable tensors: the fixture carries no fp32 rounding of its own
    trip = np.unique(np.stack([rng.integers(1, E, size=400), rng.integers(1, R, size=400), rng.integers(1, E, size=400)], 1), axis=0)
    trip = trip[rng.permutation(len(trip))]
    train, test = trip[:N_TRAIN].copy(), trip[N_TRAIN:N_TRAIN + N_TEST].copy()
    valid = trip[N_TRAIN + N_TEST:N_TRAIN + 2 * N_TEST]
    train[0, 0], train[1, 2], train[2, 1] = 0, 0, 0   # the batch: entity 0 as a head, as a tail, relation 0
    test[0, 0], test[1, 2], test[2, 1] = 0, 0, 0
    known = np.concatenate([train, valid, test])
    ids = lambda rows, col: torch.from_numpy(np.ascontiguousarray(rows[:, col]))
    # non-trivial running buffers: two training forwards on other rows, without dropout, then rounded to fp32
    model.inp_drop = model.feature_map_drop = model.hidden_drop = torch.nn.Identity()
    model.train()
    with torch.no_grad():
        model(ids(train[B:3 * B], 0), ids(train[B:3 * B], 1), direction="tail")
        model(ids(train[3 * B:5 * B], 2), ids(train[3 * B:5 * B], 1), direction="head")
        for key, v in model.state_dict().items():
            if "running" in key:
                v.copy_(v.float().double())
    rec = {"E": E, "R": R, "in_channels": C, "way": way, "first_atrous": A1, "second_atrous": A2, "third_atrous": A3,
           "acre_bias": acre_bias, "label_smoothing": -1.0 if ls is None else ls, "dropouts": np.asarray(rates, dtype=np.float64),
           "train": train, "valid": valid, "test": test, "state_keys": np.asarray(list(model.state_dict().keys()))}
    full = {}
    for key, v in model.state_dict().items():
        full[key] = v.numpy().astype(np.float32) if v.dtype.is_floating_point else v.numpy().copy()
        if v.dtype.is_floating_point:
            assert np.array_equal(full[key].astype(np.float64), v.numpy()), key
        if key in gen:
            rec["gen." + key] = np.asarray(gen[key], dtype=np.float64)
        else:
            rec[key] = full[key]
    assert tuple(k for k in rec["state_keys"] if "running" not in k and "num_batches" not in k) == ar.tensors(G), rec["state_keys"]
    P = {key: full[key].astype(np.float64) for key in ar.tensors(G) + ar.BUFFERS}
    h, r, t = (ids(train[:B], c) for c in range(3))
    assert (h == 0).sum() == 1 and (t == 0).sum() == 1 and (r == 0).any() and (test == 0).any()
    hr_t, tr_h = np.zeros((B, E), np.float64), np.zeros((B, E), np.float64)
    for i, (a, b, c) in enumerate(train[:B]):
        hr_t[i, train[(train[:, 0] == a) & (train[:, 1] == b), 2]] = 1.0
        tr_h[i, train[(train[:, 2] == c) & (train[:, 1] == b), 0]] = 1.0
    rec.update(h=h.numpy(), r=r.numpy(), t=t.numpy(), hr_t=hr_t, tr_h=tr_h)

    # ---- eval form, from the state before the step: predictions of the batch rows and the ranks of the test split
    model.eval()
    got = np.zeros((4, len(test)), dtype=np.int64)
    with torch.no_grad():
        rec["eval_pred_tails"] = model(h, r, direction="tail").numpy()
        rec["eval_pred_heads"] = model(t, r, direction="head").numpy()
        for i, (a, b, c) in enumerate(test):
            a, b, c = int(a), int(b), int(c)
            tails = model.predict_tail_rank(torch.LongTensor([a]), torch.LongTensor([b]), topk=E).view(-1).numpy()
            heads = model.predict_head_rank(torch.LongTensor([c]), torch.LongTensor([b]), topk=E).view(-1).numpy()
            got[1, i], got[3, i] = scan(tails, c, set(known[(known[:, 0] == a) & (known[:, 1] == b), 2].tolist()))
            got[0, i], got[2, i] = scan(heads, a, set(known[(known[:, 2] == c) & (known[:, 1] == b), 0].tolist()))
    rec["ranks"] = got
    want, gap = ar.ranks(P, G, test, known)
    if not gap > MIN_GAP:
        raise SystemExit("%s: a competitor lies %.3g from a true candidate (<= %g): pick another seed" % (name, gap, MIN_GAP))
    if not np.array_equal(want, got):
        raise SystemExit("%s: float64 ranks differ from the reference's:\n%s\n%s" % (name, want, got))
    close(name + " eval_pred_tails", ar.forward(P, G, rec["h"], rec["r"], "tail"), rec["eval_pred_tails"])
    close(name + " eval_pred_heads", ar.forward(P, G, rec["t"], rec["r"], "head"), rec["eval_pred_heads"])
    margin = min(ar.eval_margin(P, G, test), ar.eval_margin(P, G, train[:B]))

    # ---- the training step under known masks
    mask_list = None
    if mask_key is not None:
        mseed, moffset = mask_key
        mask_list = [ar.masks(B, G, rates, mseed, moffset, row0=side * B) for side in (0, 1)]
        for side, m in enumerate(mask_list):
            for site, x in enumerate(m):
                if not ((x == 0).any() and (x != 0).any()):
                    raise SystemExit("%s: site %d of direction %d does not both keep and drop: pick another mask key" % (name, site, side))
                rec["mask.%s.%d" % (("tail", "head")[side], site)] = x
        rec["mask_seed"], rec["mask_offset"] = np.uint64(mseed), np.uint64(moffset)
        model.inp_drop = MaskDrop([m[0] for m in mask_list], (B, 1, 20, 20))
        model.feature_map_drop = MaskDrop([m[1] for m in mask_list], (B, C, 1, 1))
        model.hidden_drop = MaskDrop([m[2] for m in mask_list], (B, K))
    model.train()
    pred_tails, pred_heads = model(h, r, direction="tail"), model(t, r, direction="head")
    loss = Criterion.multi_class_bce(pred_heads, pred_tails, torch.from_numpy(tr_h), torch.from_numpy(hr_t), ls, E if ls is not None else None)
    loss.backward()
    rec.update(pred_tails=pred_tails.detach().numpy(), pred_heads=pred_heads.detach().numpy(), loss=np.float64(loss.item()))
    out = ar.step(P, G, rec["h"], rec["r"], rec["t"], hr_t, tr_h, label_smoothing=ls, mask_list=mask_list)
    vanishing = ar.vanishing(G, rates, P)
    for key, p in model.named_parameters():
        g = p.grad.numpy().copy()
        if key in vanishing:   # zero or nearly so: rounding noise on both sides, compared on the cancellation scale
            if not np.abs(out["grads"][key] - g).max() <= RTOL * max(out["scale"][key], np.abs(g).max()):
                raise SystemExit("%s: grad.%s differs beyond its cancellation scale" % (name, key))
            print("  %s grad.%s: max-abs %.3g on a cancellation scale of %.3g" % (name, key, np.abs(g).max(), out["scale"][key]))
        else:
            close(name + " grad." + key, out["grads"][key], g)
        if key in ar.LARGE:   # a sample, the arg-max entry, the max-abs and the sum
            flat = g.reshape(-1)
            idx = np.concatenate([ar.sample_index(seed * 10 + 5, flat.size), [int(np.abs(flat).argmax())]])
            rec["grad_sample_seed." + key] = np.int64(seed * 10 + 5)
            rec["grad_index." + key], rec["grad_sample." + key] = idx, flat[idx]
            rec["grad_maxabs." + key], rec["grad_sum." + key] = np.abs(flat).max(), flat.sum()
        else:
            rec["grad." + key] = g
    for key, v in model.state_dict().items():
        if "running" in key or "num_batches" in key:
            rec["after." + key] = v.numpy().copy()
    close(name + " loss", out["loss"], rec["loss"])
    close(name + " pred_tails", out["pred_tails"], rec["pred_tails"])
    close(name + " pred_heads", out["pred_heads"], rec["pred_heads"])
    for key in ar.BUFFERS:
        close(name + " after." + key, out["buffers"][key], rec["after." + key])
    for key in ar.COUNTERS:
        assert int(rec["after." + key]) == int(rec[key]) + 2, key
    margin = min(margin, out["margin"])
    if not margin > MIN_MARGIN:
        raise SystemExit("%s: a bn1 or bn2 output lies %.3g from zero (<= %g): pick another seed" % (name, margin, MIN_MARGIN))
    path = os.path.join(OUT, "ref_%s.npz" % name)
    np.savez_compressed(path, **rec)
    print("wrote %s: loss %.9f, smallest neighbour gap %.3g, smallest pre-ReLU margin %.3g, eval predictions %.3g .. %.3g, %d bytes"
          % (name, rec["loss"], gap, margin, min(rec["eval_pred_tails"].min(), rec["eval_pred_heads"].min()),
             max(rec["eval_pred_tails"].max(), rec["eval_pred_heads"].max()), os.path.getsize(path)))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    for name, case in CASES.items():
        if not only or name in only:
            golden(name, *case)
