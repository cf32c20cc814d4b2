"""Float64 numpy restatement of ConvE (models/projection.py:12-125) with train_step_projection (utils/trainer.py:159-174) and
Criterion.multi_class_bce: the body in its training and eval forms, loss, the 13 gradients, the running-buffer updates and the ranks.
The dropout masks are the Philox masks csrc/kge_conve.hip documents, built on oracle/sampler_oracle.py:philox4x32_10 (through
tools/tucker_reference.py:mask, the same counter layout):

    key = (seed & 0xffffffff, seed >> 32);  counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff);  word = row & 3
    site 0 (input dropout): elem = pixel in [0, 2k);  site 1 (feature-map dropout): elem = channel in [0, 32);  site 2 (hidden
    dropout): elem = j in [0, k);  row = row0 + position in the call: the step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1
    keep iff word >= floor(p * 2^32) with p the float32 rate; kept elements are scaled by the float32 value 1 / (1 - p)

`dtype` selects the arithmetic (np.float64: the restatement; np.float32: the plain fp32 run whose error sets the tests' tolerances).
P: a dict with the model's state-dict keys (parameters and running buffers) and "hidden_size_1" (fc.weight's width does not determine it)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.tucker_reference import dense_labels, mask, rank64, sigmoid  # noqa: E402,F401

TENSORS = ("ent_embeddings.weight", "rel_embeddings.weight", "b.weight", "bn0.weight", "bn0.bias", "conv2d_1.weight", "conv2d_1.bias",
           "bn1.weight", "bn1.bias", "fc.weight", "fc.bias", "bn2.weight", "bn2.bias")
BUFFERS = ("bn0.running_mean", "bn0.running_var", "bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")
COUNTERS = ("bn0.num_batches_tracked", "bn1.num_batches_tracked", "bn2.num_batches_tracked")
VANISHING = ("bn0.weight", "bn0.bias", "conv2d_1.bias", "fc.bias")   # zero without dropout: a training-mode batch norm follows each
EPS, MOMENTUM, CH = 1e-5, 0.1, 32


def geometry(k, h1):
    """(H, W, OH, OW, F) of the stacked image and the conv output."""
    H, W = 2 * (k // h1), h1
    return H, W, H - 2, W - 2, CH * (H - 2) * (W - 2)


def masks(n, k, dropouts, seed=0, offset=0, row0=0, train=True):
    """(m0 [n, 2k], m1 [n, 32], m2 [n, k]) of the rows row0 .. row0 + n - 1."""
    if not train:
        dropouts = (0.0, 0.0, 0.0)
    return tuple(mask(site, row0 + n, elems, dropouts[site], seed, offset)[row0:] for site, elems in ((0, 2 * k), (1, CH), (2, k)))


def _bn(x, axes, w, b, dtype):
    """Training-mode batch norm over `axes`: (y, xh, mean, biased var, rstd, count)."""
    cnt = int(np.prod([x.shape[a] for a in axes]))
    mean = x.mean(axis=axes, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(axis=axes, keepdims=True, dtype=dtype)
    rstd = dtype(1.0) / np.sqrt(var + dtype(EPS))
    xh = (x - mean) * rstd
    return xh * w + b, xh, mean, var, rstd, cnt


def body(P, e, r, side, m=None, train=True, dtype=np.float64):
    """x [n, k] of one direction, what the backward needs, and (training form) the batch statistics {bn: (mean, unbiased var)}."""
    T = {key: np.asarray(P[key], dtype=dtype) for key in TENSORS + BUFFERS}
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    n, k = len(e), ent.shape[1]
    R = rel.shape[0] // 2
    if m is None:
        m = masks(n, k, (0, 0, 0))
    m0, m1, m2 = (np.asarray(x, dtype=dtype) for x in m)
    H, W, OH, OW, F = geometry(k, int(P["hidden_size_1"]))
    assert T["fc.weight"].shape == (k, F), (T["fc.weight"].shape, k, F)
    img = np.concatenate([ent[e], rel[np.asarray(r) + side * R]], 1)                      # [n, 2k]: the entity half first
    s = dict(img=img, n=n)
    stats = {}
    w0, b0 = T["bn0.weight"][0], T["bn0.bias"][0]
    if train:
        y0, s["xh0"], mean, var, s["rstd0"], cnt = _bn(img, (0, 1), w0, b0, dtype)
        stats["bn0"] = (mean.reshape(1), var.reshape(1) * dtype(cnt) / dtype(cnt - 1))
    else:
        y0 = (img - T["bn0.running_mean"][0]) / np.sqrt(T["bn0.running_var"][0] + dtype(EPS)) * w0 + b0
    y0d = (y0 * m0).reshape(n, H, W)
    patches = np.stack([y0d[:, dy:dy + OH, dx:dx + OW] for dy in range(3) for dx in range(3)], 1)   # [n, 9, OH, OW]
    cw = T["conv2d_1.weight"].reshape(CH, 9)
    c = np.einsum("cq,nqyx->ncyx", cw, patches) + T["conv2d_1.bias"][None, :, None, None]
    w1, b1 = T["bn1.weight"][None, :, None, None], T["bn1.bias"][None, :, None, None]
    if train:
        y1, s["xh1"], mean, var, s["rstd1"], cnt = _bn(c, (0, 2, 3), w1, b1, dtype)
        stats["bn1"] = (mean.reshape(CH), var.reshape(CH) * dtype(cnt) / dtype(cnt - 1))
    else:
        y1 = (c - T["bn1.running_mean"][None, :, None, None]) / np.sqrt(T["bn1.running_var"][None, :, None, None] + dtype(EPS)) * w1 + b1
    A = (np.maximum(y1, 0) * m1[:, :, None, None]).reshape(n, F)
    u = A @ T["fc.weight"].T + T["fc.bias"]
    s.update(patches=patches, y1=y1, A=A, u=u, m=(m0, m1, m2), geom=(H, W, OH, OW, F))
    if train:
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        y2, s["xh2"], mean, var, s["rstd2"], cnt = _bn(u * m2, (0,), T["bn2.weight"], T["bn2.bias"], dtype)
        stats["bn2"] = (mean.reshape(k), var.reshape(k) * dtype(n) / dtype(n - 1))
        s["y2"] = y2
        x = np.maximum(y2, 0)
    else:
        x = np.maximum(u, 0)   # bn2 is skipped under eval() (`if self.training:`), and no dropout is drawn
    return x, s, stats


def body_backward(P, e, r, side, s, dx, dtype=np.float64):
    """The 13 gradients of one direction's training-form body given dx (b.weight: zero, it is the head's), and the cancellation scale
    (sum of the absolute summands) of the four gradients that vanish without dropout."""
    T = {key: np.asarray(P[key], dtype=dtype) for key in TENSORS}
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    n, k, R = s["n"], ent.shape[1], rel.shape[0] // 2
    H, W, OH, OW, F = s["geom"]
    m0, m1, m2 = s["m"]
    g, scale = {}, {}

    def bn_back(dy, xh, w, rstd, axes):
        cnt = dtype(np.prod([dy.shape[a] for a in axes]))
        S1, S2 = dy.sum(axis=axes, keepdims=True), (dy * xh).sum(axis=axes, keepdims=True)
        return w * rstd * (dy - S1 / cnt - xh * (S2 / cnt)), S1, S2

    dy2 = dx * (s["y2"] > 0)
    dud, S1, S2 = bn_back(dy2, s["xh2"], T["bn2.weight"], s["rstd2"], (0,))
    g["bn2.weight"], g["bn2.bias"] = S2.reshape(k), S1.reshape(k)
    du = dud * m2
    g["fc.bias"], scale["fc.bias"] = du.sum(0), np.abs(du).sum(0).max()
    g["fc.weight"] = du.T @ s["A"]
    dy1 = ((du @ T["fc.weight"]).reshape(n, CH, OH, OW) * m1[:, :, None, None]) * (s["y1"] > 0)
    dc, S1, S2 = bn_back(dy1, s["xh1"], T["bn1.weight"][None, :, None, None], s["rstd1"], (0, 2, 3))
    g["bn1.weight"], g["bn1.bias"] = S2.reshape(CH), S1.reshape(CH)
    g["conv2d_1.bias"], scale["conv2d_1.bias"] = dc.sum((0, 2, 3)), np.abs(dc).sum((0, 2, 3)).max()
    g["conv2d_1.weight"] = np.einsum("ncyx,nqyx->cq", dc, s["patches"]).reshape(CH, 1, 3, 3)
    cw = T["conv2d_1.weight"].reshape(CH, 3, 3)
    dy0d = np.zeros((n, H, W), dtype=dtype)
    for dy in range(3):
        for dx_ in range(3):
            dy0d[:, dy:dy + OH, dx_:dx_ + OW] += np.einsum("ncyx,c->nyx", dc, cw[:, dy, dx_])
    dy0 = dy0d.reshape(n, 2 * k) * m0
    dimg, S1, S2 = bn_back(dy0, s["xh0"], T["bn0.weight"][0], s["rstd0"], (0, 1))
    g["bn0.weight"], g["bn0.bias"] = S2.reshape(1), S1.reshape(1)
    scale["bn0.weight"], scale["bn0.bias"] = np.abs(dy0 * s["xh0"]).sum(), np.abs(dy0).sum()
    g["ent_embeddings.weight"], g["rel_embeddings.weight"] = np.zeros_like(ent), np.zeros_like(rel)
    np.add.at(g["ent_embeddings.weight"], e, dimg[:, :k])
    np.add.at(g["rel_embeddings.weight"], np.asarray(r) + side * R, dimg[:, k:])
    g["b.weight"] = np.zeros_like(T["b.weight"])
    return g, {key: float(v) for key, v in scale.items()}


def update_buffers(buffers, stats, dtype=np.float64):
    """running = (1 - momentum) running + momentum (mean, unbiased variance), in place on the dict of running buffers."""
    for bn, (mean, var) in stats.items():
        buffers[bn + ".running_mean"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_mean"] + dtype(MOMENTUM) * mean
        buffers[bn + ".running_var"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_var"] + dtype(MOMENTUM) * var


def forward(P, e, r, direction="tail", m=None, train=False, dtype=np.float64):
    """[n, E] predictions of ConvE.forward (no buffer update)."""
    x, _, _ = body(P, e, r, 0 if direction == "tail" else 1, m, train, dtype)
    return sigmoid(x @ np.asarray(P["ent_embeddings.weight"], dtype=dtype).T + np.asarray(P["b.weight"], dtype=dtype))


def step(P, h, r, t, y_hr_t, y_tr_h, dropouts=(0.0, 0.0, 0.0), seed=0, offset=0, label_smoothing=None, dtype=np.float64, mask_list=None):
    """One train_step_projection: dict(loss, grads, pred_tails, pred_heads, buffers (after the step: updated tail first, then head),
    scale (cancellation scales of VANISHING), margin (smallest |pre-ReLU value| of bn1 / bn2 outputs)).  y_*: dense multi-hot label
    rows [B, E].  mask_list: ((m0, m1, m2) of the tail direction, of the head direction) instead of the Philox masks."""
    ent = np.asarray(P["ent_embeddings.weight"], dtype=dtype)
    bias = np.asarray(P["b.weight"], dtype=dtype)
    E, k = ent.shape
    B = len(h)
    buffers = {key: np.asarray(P[key], dtype=dtype).copy() for key in BUFFERS}
    grads = {key: np.zeros_like(np.asarray(P[key], dtype=dtype)) for key in TENSORS}
    scale = {key: 0.0 for key in VANISHING}
    loss, preds, margin = dtype(0), [], np.inf
    for side, (ee, yy) in enumerate(((h, y_hr_t), (t, y_tr_h))):
        m = mask_list[side] if mask_list is not None else masks(B, k, dropouts, seed, offset, row0=side * B)
        x, s, stats = body(P, ee, r, side, m, True, dtype)
        update_buffers(buffers, stats, dtype)
        margin = min(margin, np.abs(s["y1"]).min(), np.abs(s["y2"]).min())
        p = sigmoid(x @ ent.T + bias)
        Y = np.asarray(yy, dtype=dtype)
        if label_smoothing is not None:
            Y = Y * dtype(1.0 - label_smoothing) + dtype(1.0 / E)
        # BCEWithLogits applied to the sigmoid outputs (sic): softplus(p) - y p, mean over B * E per direction, the two added
        loss = loss + (np.log1p(np.exp(p)) - Y * p).sum() / dtype(B * E)
        dlogit = (sigmoid(p) - Y) / dtype(B * E) * p * (1 - p)
        g, sc = body_backward(P, ee, r, side, s, dlogit @ ent, dtype)
        for key in TENSORS:
            grads[key] = grads[key] + g[key]
        grads["ent_embeddings.weight"] = grads["ent_embeddings.weight"] + dlogit.T @ x
        grads["b.weight"] = grads["b.weight"] + dlogit.sum(0, keepdims=True)
        for key in VANISHING:
            scale[key] += sc[key]
        preds.append(p)
    return dict(loss=float(loss), grads=grads, pred_tails=preds[0], pred_heads=preds[1], buffers=buffers, scale=scale, margin=float(margin))


def ranks(P, test, known):
    """int [4, n]: rank_head, rank_tail, filtered_rank_head, filtered_rank_tail (0-based) of the test triples in the eval form, float64,
    plus the smallest distance of another candidate's prediction to the true one's."""
    test = np.asarray(test)
    out = np.zeros((4, len(test)), dtype=np.int64)
    gap = np.inf
    pts = forward(P, test[:, 0], test[:, 1], "tail")
    phs = forward(P, test[:, 2], test[:, 1], "head")
    for i, (h, r, t) in enumerate(test):
        pt, ph = pts[i], phs[i]
        out[1, i], out[3, i] = rank64(pt, t, known[(known[:, 0] == h) & (known[:, 1] == r), 2])
        out[0, i], out[2, i] = rank64(ph, h, known[(known[:, 2] == t) & (known[:, 1] == r), 0])
        gap = min(gap, np.abs(np.delete(pt, t) - pt[t]).min(), np.abs(np.delete(ph, h) - ph[h]).min())
    return out, gap


def adam_trajectory(P, batches, lr, dropouts, seed, label_smoothing, dtype=np.float64, optimizer="adam"):
    """`len(batches)` Adam steps (torch defaults: betas 0.9 / 0.999, eps 1e-8; optimizer="sgd": plain SGD steps instead) of the fused step
    with the Philox masks of (seed, step):
    (per-step losses, final P with the running buffers, smallest pre-ReLU margin over the steps)."""
    P = {key: np.asarray(v, dtype=dtype).copy() for key, v in P.items() if key in TENSORS + BUFFERS + ("hidden_size_1",)}
    m1 = {key: np.zeros_like(P[key]) for key in TENSORS}
    m2 = {key: np.zeros_like(P[key]) for key in TENSORS}
    losses, margin = [], np.inf
    for i, (h, r, t, y1, y2) in enumerate(batches):
        out = step(P, h, r, t, y1, y2, dropouts=dropouts, seed=seed, offset=i, label_smoothing=label_smoothing, dtype=dtype)
        losses.append(out["loss"])
        margin = min(margin, out["margin"])
        P.update(out["buffers"])
        for key in TENSORS:
            g = out["grads"][key]
            if optimizer == "sgd":
                P[key] = P[key] - dtype(lr) * g
                continue
            # the optimiser's formulas as csrc/kge_opt_device.h states them (torch's _single_tensor_adam): the weights 1 - beta are
            # formed in the run's own precision (in fp32, 1 - 0.999 is 1.3e-5 off 0.001), the bias corrections in double
            m1[key] = m1[key] + (dtype(1) - dtype(0.9)) * (g - m1[key])
            m2[key] = m2[key] * dtype(0.999) + (dtype(1) - dtype(0.999)) * g * g
            denom = np.sqrt(m2[key]) / dtype(np.sqrt(1 - 0.999 ** (i + 1))) + dtype(1e-8)
            P[key] = P[key] - dtype(lr / (1 - 0.9 ** (i + 1))) * m1[key] / denom
    return losses, P, margin
