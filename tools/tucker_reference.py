"""Float64 numpy restatement of TuckER (models/projection.py:259-344) with train_step_projection (utils/trainer.py:159-172) and
Criterion.multi_class_bce: forward, loss, the three gradients and the ranks.  The dropout masks are the Philox masks csrc/kge_tucker.hip
documents, built on oracle/sampler_oracle.py:philox4x32_10:

    key = (seed & 0xffffffff, seed >> 32);  counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff);  word = row & 3
    elem = i (site 0: input dropout), i * d1 + j (site 1: hidden dropout 1), j (site 2: hidden dropout 2)
    keep iff word >= floor(p * 2^32) with p the float32 rate; kept elements are scaled by the float32 value 1 / (1 - p)

`dtype` selects the arithmetic (np.float64: the restatement; np.float32: the plain fp32 run whose error sets the tests' tolerances)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from sampler_oracle import philox4x32_10  # noqa: E402

EPS = 1e-12


def mask(site, rows, elems, p, seed=0, offset=0):
    """float64 [rows, elems]: 0 or the fp32 scale 1 / (1 - p) for every (row, element) of `site`; all ones for p == 0."""
    p32 = np.float32(p)
    if p32 == 0:
        return np.ones((rows, elems))
    thr = int(np.floor(float(p32) * 2.0 ** 32))
    scale = float(np.float32(1.0) / (np.float32(1.0) - p32))
    grp = (rows + 3) // 4
    c0 = np.tile(np.arange(elems, dtype=np.uint64), grp)
    c1 = np.repeat(np.arange(grp, dtype=np.uint64), elems)
    c2 = np.full(c0.shape, (site | ((offset >> 32) << 2)) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(c0.shape, offset & 0xFFFFFFFF, dtype=np.uint64)
    words = philox4x32_10((c0, c1, c2, c3), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))   # elementwise on uint64 arrays
    words = np.stack(words, 1).reshape(grp, elems, 4).transpose(0, 2, 1).reshape(grp * 4, elems)[:rows]
    return np.where(words >= thr, scale, 0.0)


def masks(n, d1, dropouts, seed=0, offset=0, train=True):
    if not train:
        dropouts = (0.0, 0.0, 0.0)
    return (mask(0, n, d1, dropouts[0], seed, offset), mask(1, n, d1 * d1, dropouts[1], seed, offset).reshape(n, d1, d1),
            mask(2, n, d1, dropouts[2], seed, offset))


def body(P, e, r, m, dtype=np.float64):
    """x [n, d1] and what the backward needs."""
    ent, rel, W = (np.asarray(P[k], dtype=dtype) for k in ("ent_embeddings.weight", "rel_embeddings.weight", "W.weight"))
    d1, d2 = ent.shape[1], rel.shape[1]
    m0, m1, m2 = (np.asarray(x, dtype=dtype) for x in m)
    rows = ent[e]
    na = np.sqrt((rows * rows).sum(1, keepdims=True))
    a = rows / np.maximum(na, dtype(EPS)) * m0
    M = (rel[r] @ W.reshape(d2, d1 * d1)).reshape(-1, d1, d1) * m1
    z = np.einsum("bi,bij->bj", a, M)
    nz = np.sqrt((z * z).sum(1, keepdims=True))
    x = z / np.maximum(nz, dtype(EPS)) * m2
    return x, dict(rows=rows, na=na, a=a, M=M, z=z, nz=nz)


def body_backward(P, e, r, m, saved, dx, dtype=np.float64):
    ent, rel, W = (np.asarray(P[k], dtype=dtype) for k in ("ent_embeddings.weight", "rel_embeddings.weight", "W.weight"))
    d1, d2 = ent.shape[1], rel.shape[1]
    m0, m1, m2 = (np.asarray(x, dtype=dtype) for x in m)
    s = saved
    den = np.maximum(s["nz"], dtype(EPS))
    g = dx * m2
    xh = s["z"] / den
    dz = (g - xh * np.where(s["nz"] >= EPS, (xh * g).sum(1, keepdims=True), 0)) / den
    G = s["a"][:, :, None] * dz[:, None, :] * m1
    Gf = G.reshape(-1, d1 * d1)
    gW = rel[r].T @ Gf
    g_rel = np.zeros_like(rel)
    np.add.at(g_rel, r, Gf @ W.reshape(d2, d1 * d1).T)
    ga = np.einsum("bij,bj->bi", s["M"], dz) * m0
    dena = np.maximum(s["na"], dtype(EPS))
    ah = s["rows"] / dena
    g_rows = (ga - ah * np.where(s["na"] >= EPS, (ah * ga).sum(1, keepdims=True), 0)) / dena
    g_ent = np.zeros_like(ent)
    np.add.at(g_ent, e, g_rows)
    return {"ent_embeddings.weight": g_ent, "rel_embeddings.weight": g_rel, "W.weight": gW.reshape(d2, d1 * d1)}


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(P, e, r, m=None, dtype=np.float64):
    """[n, E] predictions of TuckER.forward."""
    n, d1 = len(e), np.asarray(P["ent_embeddings.weight"]).shape[1]
    if m is None:
        m = masks(n, d1, (0, 0, 0))
    x, _ = body(P, e, r, m, dtype)
    return sigmoid(x @ np.asarray(P["ent_embeddings.weight"], dtype=dtype).T)


def dense_labels(off, ids, E):
    y = np.zeros((len(off) - 1, E))
    for i in range(len(off) - 1):
        y[i, ids[off[i]:off[i + 1]]] = 1.0
    return y


def step(P, h, r, t, y_hr_t, y_tr_h, dropouts=(0.0, 0.0, 0.0), seed=0, offset=0, label_smoothing=None, train=True, dtype=np.float64):
    """(loss, gradients, pred_tails, pred_heads) of one train_step_projection.  Rows [h; t] share one mask draw, as the fused step does;
    y_*: dense multi-hot label rows [B, E]."""
    ent = np.asarray(P["ent_embeddings.weight"], dtype=dtype)
    E, d1 = ent.shape
    B = len(h)
    e, rr = np.concatenate([h, t]), np.concatenate([r, r])
    m = masks(2 * B, d1, dropouts, seed, offset, train)
    x, saved = body(P, e, rr, m, dtype)
    p = sigmoid(x @ ent.T)
    Y = np.concatenate([y_hr_t, y_tr_h]).astype(dtype)
    if label_smoothing is not None:
        Y = Y * dtype(1.0 - label_smoothing) + dtype(1.0 / E)
    # BCEWithLogits applied to the sigmoid outputs (sic): softplus(p) - y p, mean over B * E per direction, the two added
    loss = (np.log1p(np.exp(p)) - Y * p).sum() / dtype(B * E)
    dp = (sigmoid(p) - Y) / dtype(B * E)
    dlogit = dp * p * (1 - p)
    g = body_backward(P, e, rr, m, saved, dlogit @ ent, dtype)
    g["ent_embeddings.weight"] = g["ent_embeddings.weight"] + dlogit.T @ x
    return float(loss), g, p[:B], p[B:]


def rank64(row, true, known):
    """(rank, filtered rank) of entity `true` in the prediction row: the number of entities predicted strictly above it
    (utils/evaluator.py:70-123 walks topk(-preds) from its end), without the known ones for the filtered rank."""
    above = row > row[true]
    rank = int(above.sum())
    known = np.asarray([k for k in set(int(x) for x in known) if k != true], dtype=np.int64)
    return rank, rank - int(above[known].sum()) if len(known) else rank


def ranks(P, test, known):
    """int [4, n]: rank_head, rank_tail, filtered_rank_head, filtered_rank_tail (0-based) of the test triples, float64, plus the smallest
    distance of another candidate's prediction to the true one's."""
    out = np.zeros((4, len(test)), dtype=np.int64)
    gap = np.inf
    for i, (h, r, t) in enumerate(test):
        pt = forward(P, np.array([h]), np.array([r]))[0]
        ph = forward(P, np.array([t]), np.array([r]))[0]
        out[1, i], out[3, i] = rank64(pt, t, known[(known[:, 0] == h) & (known[:, 1] == r), 2])
        out[0, i], out[2, i] = rank64(ph, h, known[(known[:, 2] == t) & (known[:, 1] == r), 0])
        gap = min(gap, np.abs(np.delete(pt, t) - pt[t]).min(), np.abs(np.delete(ph, h) - ph[h]).min())
    return out, gap
