"""Numpy restatement of the triple-classification contract (include/kge_hip.h: kge_classification_fit / _apply, kge_corrupt_typed) --
TEST INFRASTRUCTURE.  Plain and slow on purpose: the fit tries every valid cut of every relation, the AUC counts walk the tie groups,
the typed draw replays the device's Philox stream through oracle/sampler_oracle.py."""
import numpy as np
import torch

import sampler_oracle as so

NAN_KEY = 0xFFFFFFFF
TYPED_ATTEMPTS, UNIFORM_ATTEMPTS = 16, 64


def keys_of(scores, higher_is_better):
    """int64 keys: smaller = more plausible; -0.0 == +0.0; every NaN is NAN_KEY, above every number."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    bits = s.view(np.uint32).astype(np.int64)
    bits = np.where(bits == 0x80000000, 0, bits)
    asc = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
    key = (~asc & 0xFFFFFFFF) if higher_is_better else asc
    return np.where(np.isnan(s), NAN_KEY, key).astype(np.int64)


def positive(key, thr):
    return (key != NAN_KEY) & (key <= thr)


def fit(scores, rel, label, R, higher_is_better):
    """(thr int64 [R], fit int64 [R, 6]): per relation every cut is tried -- before everything (-1) and at every distinct number key,
    in ascending order -- and the first one with the most correct triples wins; wins / ties per distinct negative key."""
    key = keys_of(scores, higher_is_better)
    rel, lab = np.asarray(rel, dtype=np.int64), np.asarray(label) != 0
    thr = np.full(R, -1, dtype=np.int64)
    out = np.zeros((R, 6), dtype=np.int64)
    for r in range(R):
        m = rel == r
        k, l = key[m], lab[m]
        kp, kn = k[l], k[~l]
        best, best_cut = len(kn), -1                     # the cut before everything: every negative is right
        for c in np.unique(k[k != NAN_KEY]):
            p = positive(k, c)
            correct = int((p & l).sum() + (~p & ~l).sum())
            if correct > best:
                best, best_cut = correct, int(c)
        wins = ties = 0
        for v in np.unique(kn):
            cnt = int((kn == v).sum())
            wins += cnt * int((kp < v).sum())
            ties += cnt * int((kp == v).sum())
        thr[r] = best_cut
        out[r] = (len(kp), len(kn), best if len(k) else 0, wins, ties, 0)
    return thr, out


def apply(scores, rel, thr, seen, thr_global, label, higher_is_better):
    """(pred uint8 [n], conf int64 [R, 4] = {tp, fp, tn, fn} or None)."""
    key = keys_of(scores, higher_is_better)
    rel = np.asarray(rel, dtype=np.int64)
    thr, seen = np.asarray(thr, dtype=np.int64), np.asarray(seen) != 0
    R = len(thr)
    ok = (rel >= 0) & (rel < R)
    rc = np.where(ok, rel, 0)
    pred = ok & positive(key, np.where(seen[rc], thr[rc], thr_global))
    if label is None:
        return pred.astype(np.uint8), None
    lab = np.asarray(label) != 0
    conf = np.zeros((R, 4), dtype=np.int64)
    cell = np.where(lab, np.where(pred, 0, 3), np.where(pred, 1, 2))
    np.add.at(conf, (rc[ok], cell[ok]), 1)
    return pred.astype(np.uint8), conf


def type_lists(train, R):
    """(type_off int64 [2, R + 1], type_ids int32): row 0 = the heads seen with each relation, row 1 = the tails, ascending."""
    train = np.asarray(train, dtype=np.int64).reshape(-1, 3)
    off = np.zeros((2, R + 1), dtype=np.int64)
    ids = []
    for side, col in ((0, 0), (1, 2)):
        for r in range(R):
            off[side, r] = len(ids)
            ids.extend(sorted(set(train[train[:, 1] == r][:, col].tolist())))
        off[side, R] = len(ids)
    return off, np.asarray(ids, dtype=np.int32)


def corrupt_typed(ph, pr, pt, E, R, bern, type_off, type_ids, known, seed, offset):
    """(neg int64 [n, 3], failed rows, fell_back bool [n]): the draw of kge_corrupt_typed.  known: a set of (h, r, t) or None.
    fell_back[i]: the accepted entity came from a uniform draw (or nothing was accepted)."""
    n = len(ph)
    neg = np.zeros((n, 3), dtype=np.int64)
    fell = np.zeros(n, dtype=bool)
    failed = 0
    for i in range(n):
        h, r, t = int(ph[i]), int(pr[i]), int(pt[i])
        ctr = offset + i
        key = (seed & so.MASK32, (seed >> 32) & so.MASK32)
        base = (ctr & so.MASK32, (ctr >> 32) & so.MASK32)
        x = so.philox4x32_10(base + (0, 0), key)
        u = np.float32(x[0] >> 8) * np.float32(1.0 / 16777216.0)
        tail = bool(u > np.float32(0.5 if bern is None else bern[r]))
        lo, hi = int(type_off[1 if tail else 0, r]), int(type_off[1 if tail else 0, r + 1])
        typed = TYPED_ATTEMPTS if hi > lo else 0
        e = -1
        for a in range(typed + UNIFORM_ATTEMPTS):
            if a:
                x = so.philox4x32_10(base + (a, 0), key)
            c = int(type_ids[lo + ((x[1] * (hi - lo)) >> 32)]) if a < typed else (x[1] * E) >> 32
            if c != (t if tail else h) and (known is None or ((h, r, c) if tail else (c, r, t)) not in known):
                e, fell[i] = c, a >= typed
                break
        if e < 0:
            failed += 1
            fell[i] = True
        neg[i] = (h, r, e) if tail else (e, r, t)
    return neg, failed, fell


def metrics(conf, fit_rows):
    """The dict Evaluator.test_classification returns (without n_dropped), in plain python arithmetic."""
    R = len(conf)
    acc, auc = np.full(R, np.nan), np.full(R, np.nan)
    right = tot = num = den = 0
    for r in range(R):
        tp, fp, tn, fn = map(int, conf[r])
        if tp + fp + tn + fn:
            acc[r] = (tp + tn) / (tp + fp + tn + fn)
        right, tot = right + tp + tn, tot + tp + fp + tn + fn
        p, q, w, t = int(fit_rows[r][0]), int(fit_rows[r][1]), int(fit_rows[r][3]), int(fit_rows[r][4])
        if p * q:
            auc[r] = (2 * w + t) / (2 * p * q)
        num, den = num + 2 * w + t, den + 2 * p * q
    return {"accuracy": right / tot if tot else float("nan"), "accuracy_per_relation": acc, "auc": num / den if den else float("nan"),
            "auc_per_relation": auc, "confusion": np.asarray(conf, dtype=np.int64)}


def same_metrics(a, b):
    return (a["accuracy"] == b["accuracy"] and a["auc"] == b["auc"] and np.array_equal(a["confusion"], b["confusion"])
            and np.array_equal(a["accuracy_per_relation"], b["accuracy_per_relation"], equal_nan=True)
            and np.array_equal(a["auc_per_relation"], b["auc_per_relation"], equal_nan=True))


# ---- the three kernel calls as a torch-tensor backend (what Evaluator expects from pykg2vec_amd.kernels), for the CPU plumbing tests
def classification_fit_torch(scores, rel, label, n_relations, higher_is_better=False):
    thr, rows = fit(scores.numpy(), rel.numpy(), label.numpy(), int(n_relations), higher_is_better)
    return torch.from_numpy(thr), torch.from_numpy(rows)


def classification_apply_torch(scores, rel, thr, seen, thr_global, label=None, higher_is_better=False):
    pred, conf = apply(scores.numpy(), rel.numpy(), thr.numpy(), seen.numpy(), int(thr_global), None if label is None else label.numpy(),
                       higher_is_better)
    return torch.from_numpy(pred), None if conf is None else torch.from_numpy(conf)


def corrupt_typed_torch(ph, pr, pt, tot_entity, tot_relation, bern_prob, type_off, type_ids, slots, seed, offset):
    neg, failed, _ = corrupt_typed(ph.numpy(), pr.numpy(), pt.numpy(), int(tot_entity), int(tot_relation),
                                   None if bern_prob is None else bern_prob.numpy(), type_off.numpy(), type_ids.numpy(), slots, int(seed), int(offset))
    return torch.from_numpy(neg), torch.tensor([failed], dtype=torch.int64)
