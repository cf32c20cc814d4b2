"""Numpy restatement of ProjE_pointwise (models/projection.py:128-257) with train_step_projection (utils/trainer.py:159-174): both
direction losses, the regulariser, the eight gradients and the ranks.  The labels are dense rows in {-1, 0, +1} as the reference's
generator builds them (data/generator.py:161-241).  The dropout masks are the Philox masks csrc/kge_proje.hip documents -- TuckER's
scheme (tools/tucker_reference.py: mask) with site = the side (0: the tail direction's f1, 1: the head direction's f2), elem = the
column of x and row = the row's index in its own direction's list:

    key = (seed & 0xffffffff, seed >> 32);  counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff);  word = row & 3
    keep iff word >= floor(p * 2^32) with p the float32 rate; kept elements are scaled by the float32 value 1 / (1 - p)

`dtype` selects the arithmetic (np.float64: the restatement; np.float32: the plain fp32 run whose error sets the tests' tolerances)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tucker_reference import mask, rank64  # noqa: E402,F401  (mask(site, rows, elems, p, seed, offset): float64 [rows, elems])

TABLES = ("ent_embeddings.weight", "rel_embeddings.weight", "bc1.weight", "De1.weight", "Dr1.weight", "bc2.weight", "De2.weight",
          "Dr2.weight")   # parameter_list order
CLAMP = 1e-10


def side_tables(side):
    s = "2" if side else "1"
    return "bc%s.weight" % s, "De%s.weight" % s, "Dr%s.weight" % s


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def body(P, e, r, side, m=None, dtype=np.float64):
    """(x, y) [n, k]: y = tanh(ent[e] o De_s + rel[r] o Dr_s + bc_s), x = y * m."""
    bc, De, Dr = (np.asarray(P[k], dtype=dtype).reshape(1, -1) for k in side_tables(side))
    ent, rel = np.asarray(P[TABLES[0]], dtype=dtype), np.asarray(P[TABLES[1]], dtype=dtype)
    y = np.tanh(ent[e] * De + rel[r] * Dr + bc)
    return (y if m is None else y * np.asarray(m, dtype=dtype)), y


def label_loss(x, ent, Y, dtype=np.float64):
    """(loss, dz, logits) of the label rows Y [n, E] in {-1, 0, +1} given the body's output x [n, k]: what kge_proje_label_loss
    computes on the labelled columns.  dx = dz @ ent, and ent's gradient from the product is dz.T @ x."""
    x, ent = np.asarray(x, dtype=dtype), np.asarray(ent, dtype=dtype)
    z = x @ ent.T
    s = sigmoid(z)
    u = dtype(1) - s
    pos, neg = np.maximum(Y, 0).astype(dtype), np.maximum(-Y, 0).astype(dtype)
    c = dtype(CLAMP)
    loss = -(np.log(np.maximum(s, c)) * pos).sum() - (np.log(np.maximum(u, c)) * neg).sum()
    dz = pos * np.where(s > c, -u, 0) + neg * np.where(u > c, s, 0)   # clamp passes no gradient outside its range
    return loss, dz.astype(dtype), z


def direction(P, e, r, Y, side, m=None, dtype=np.float64):
    """(loss, gradients, logits) of ProjE_pointwise.forward(e, r, Y, direction) with Y the dense label rows [n, E]."""
    ent, rel = np.asarray(P[TABLES[0]], dtype=dtype), np.asarray(P[TABLES[1]], dtype=dtype)
    kbc, kDe, kDr = side_tables(side)
    De, Dr = np.asarray(P[kDe], dtype=dtype).reshape(1, -1), np.asarray(P[kDr], dtype=dtype).reshape(1, -1)
    mm = np.ones((len(e), ent.shape[1]), dtype=dtype) if m is None else np.asarray(m, dtype=dtype)
    x, y = body(P, e, r, side, mm, dtype)
    loss, dz, z = label_loss(x, ent, Y, dtype)
    dpre = (dz @ ent) * mm * (dtype(1) - y * y)
    g = {k: np.zeros_like(np.asarray(P[k], dtype=dtype)) for k in TABLES}
    g[TABLES[0]] += dz.T @ x
    np.add.at(g[TABLES[0]], e, dpre * De)
    np.add.at(g[TABLES[1]], r, dpre * Dr)
    g[kDe] += (dpre * ent[e]).sum(0).reshape(g[kDe].shape)
    g[kDr] += (dpre * rel[r]).sum(0).reshape(g[kDr].shape)
    g[kbc] += dpre.sum(0).reshape(g[kbc].shape)
    return loss, g, z


def get_reg(P, lmbda, dtype=np.float64):
    """(lmbda * sum |w| over ent, rel, De1, Dr1, De2, Dr2, its gradients lmbda * sign(w)); bc1 / bc2 are not regularised."""
    reg = dtype(0)
    g = {}
    for k in TABLES:
        w = np.asarray(P[k], dtype=dtype)
        if k.startswith("bc"):
            g[k] = np.zeros_like(w)
            continue
        reg = reg + np.abs(w).sum()
        g[k] = dtype(lmbda) * np.sign(w)
    return dtype(lmbda) * reg, g


def masks(B, k, p, seed=0, offset=0):
    """The fused step's two masks: (tail direction, head direction), each [B, k]."""
    return mask(0, B, k, p, seed, offset), mask(1, B, k, p, seed, offset)


def step(P, h, r, t, y_hr_t, y_tr_h, lmbda, p=0.0, seed=0, offset=0, explicit_masks=None, dtype=np.float64):
    """One train_step_projection: forward(h, r, y_hr_t, "tail") + forward(t, r, y_tr_h, "head") + get_reg.  Returns a dict with
    loss_tail, loss_head, reg, loss, grads {name: array} and the logits of both directions.  explicit_masks: (m_tail, m_head)
    instead of the Philox masks of (p, seed, offset)."""
    k = np.asarray(P[TABLES[0]]).shape[1]
    m = explicit_masks if explicit_masks is not None else masks(len(h), k, p, seed, offset)
    lt, gt, zt = direction(P, h, r, y_hr_t, 0, m[0], dtype)
    lh, gh, zh = direction(P, t, r, y_tr_h, 1, m[1], dtype)
    reg, gr = get_reg(P, lmbda, dtype)
    return {"loss_tail": float(lt), "loss_head": float(lh), "reg": float(reg), "loss": float(lt + lh + reg),
            "grads": {name: gt[name] + gh[name] + gr[name] for name in TABLES}, "logits_tail": zt, "logits_head": zh}


def dense_labels(off, ids, E, neg=None):
    """The reference's label rows from a positive CSR and the batch's negative ids: +1 on the positives, -1 on the negatives that are
    no positive of the row."""
    y = np.zeros((len(off) - 1, E))
    for i in range(len(off) - 1):
        if neg is not None:
            y[i, np.asarray(neg, dtype=np.int64)] = -1.0
        y[i, ids[off[i]:off[i + 1]]] = 1.0
    return y


def predictions(P, e, r, side):
    """float64 [n, E]: sigmoid(f_s(e, r) @ ent.T) without dropout, what predict_tail_rank (side 0) / predict_head_rank (side 1) order."""
    x, _ = body(P, e, r, side)
    return sigmoid(x @ np.asarray(P[TABLES[0]], dtype=np.float64).T)


def ranks(P, test, known):
    """int [4, n]: rank_head, rank_tail, filtered_rank_head, filtered_rank_tail (0-based) of the test triples, float64, plus the smallest
    distance of another candidate's prediction to the true one's."""
    out = np.zeros((4, len(test)), dtype=np.int64)
    gap = np.inf
    for i, (h, r, t) in enumerate(test):
        pt = predictions(P, np.array([h]), np.array([r]), 0)[0]
        ph = predictions(P, np.array([t]), np.array([r]), 1)[0]
        out[1, i], out[3, i] = rank64(pt, t, known[(known[:, 0] == h) & (known[:, 1] == r), 2])
        out[0, i], out[2, i] = rank64(ph, h, known[(known[:, 2] == t) & (known[:, 1] == r), 0])
        gap = min(gap, np.abs(np.delete(pt, t) - pt[t]).min(), np.abs(np.delete(ph, h) - ph[h]).min())
    return out, gap
