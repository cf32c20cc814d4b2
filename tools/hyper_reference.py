"""Float64 numpy restatement of HypER (models/projection.py:508-618) with train_step_projection (utils/trainer.py:159-174) and
Criterion.multi_class_bce: the body in its training and eval forms, loss, the 13 gradients, the running-buffer updates and the ranks.
The dropout masks are the Philox masks csrc/kge_hyper.hip documents, built on oracle/sampler_oracle.py:philox4x32_10 (through
tools/tucker_reference.py:mask, the same counter layout):

    key = (seed & 0xffffffff, seed >> 32);  counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff);  word = row & 3
    site 0 (input dropout): elem = pixel in [0, D);  site 1 (feature-map dropout): elem = channel in [0, 32);  site 2 (hidden
    dropout): elem = j in [0, D);  row = row0 + position in the call: the step numbers the h rows 0 .. B-1 and the t rows B .. 2B-1
    keep iff word >= floor(p * 2^32) with p the float32 rate; kept elements are scaled by the float32 value 1 / (1 - p)

Both embeddings have padding_idx = 0: row 0 is an ordinary row in the forward, the lookup's gradient of id 0 is dropped, so
grad(rel)[0] = 0 and grad(ent)[0] is the head's share (x . ent^T) alone (`head_ent0` of step()).

`dtype` selects the arithmetic (np.float64: the restatement; np.float32: the plain fp32 run whose error sets the tests' tolerances).
P: a dict with the model's state-dict keys (parameters and running buffers)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.tucker_reference import dense_labels, mask, rank64, sigmoid  # noqa: E402,F401

TENSORS = ("b", "ent_embeddings.weight", "rel_embeddings.weight", "bn0.weight", "bn0.bias", "bn1.weight", "bn1.bias", "bn2.weight",
           "bn2.bias", "fc.weight", "fc.bias", "fc1.weight", "fc1.bias")
BUFFERS = ("bn0.running_mean", "bn0.running_var", "bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")
COUNTERS = ("bn0.num_batches_tracked", "bn1.num_batches_tracked", "bn2.num_batches_tracked")
EPS, MOMENTUM, CH, TAPS = 1e-5, 0.1, 32, 9


def vanishing(dropouts, bn0_bias=0.0):
    """The gradients that vanish analytically at these rates (compared on their cancellation scale): fc.bias when hidden dropout is
    off (bn2 subtracts the column mean of u * m2 = u); bn1.bias when feature-map and hidden dropout are both off (a constant added to a
    channel of A moves u by a constant per column); bn0.weight while bn0.bias = 0 (bn0.weight then only scales the conv output, which
    bn1 normalises away: it survives through bn1's eps alone).  bn0.bias and fc1.bias do not vanish: the per-row filter keeps bn1 from
    cancelling them."""
    out = []
    if float(np.asarray(bn0_bias).reshape(-1)[0]) == 0.0:
        out.append("bn0.weight")
    if not dropouts[2] > 0:
        out.append("fc.bias")
        if not dropouts[1] > 0:
            out.append("bn1.bias")
    return tuple(out)


VANISHING = vanishing


def masks(n, D, dropouts, seed=0, offset=0, row0=0, train=True):
    """(m0 [n, D], m1 [n, 32], m2 [n, D]) of the rows row0 .. row0 + n - 1."""
    if not train:
        dropouts = (0.0, 0.0, 0.0)
    return tuple(mask(site, row0 + n, elems, dropouts[site], seed, offset)[row0:] for site, elems in ((0, D), (1, CH), (2, D)))


def _bn(x, axes, w, b, dtype):
    """Training-mode batch norm over `axes`: (y, xh, mean, biased var, rstd, count)."""
    cnt = int(np.prod([x.shape[a] for a in axes]))
    mean = x.mean(axis=axes, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(axis=axes, keepdims=True, dtype=dtype)
    rstd = dtype(1.0) / np.sqrt(var + dtype(EPS))
    xh = (x - mean) * rstd
    return xh * w + b, xh, mean, var, rstd, cnt


def _bn_eval(x, mean, var, w, b, dtype):
    return (x - mean) / np.sqrt(var + dtype(EPS)) * w + b


def body(P, e, r, m=None, train=True, dtype=np.float64, fc_order=None, u_flip=None):
    """x [n, D] of one direction, what the backward needs, and (training form) the batch statistics {bn: (mean, unbiased var)}.
    fc_order: a permutation of the feature axis under which P["fc.weight"] is stored (the same model with its features renumbered: the
    tests use it to sum the fc product in another order).  u_flip: a seed; every element of the conv output c, of u and (in step()) of the head's dx is then left alone or moved by half an fp32 ulp (a
    factor 1, 1 + 2^-24 or 1 - 2^-24, seeded), the difference between two correctly rounded ways of forming the same sum (the batch norm that follows subtracts a mean from it): the tests use it to see
    how far an input's gradients depend on such roundings."""
    T = {key: np.asarray(P[key], dtype=dtype) for key in TENSORS + BUFFERS}
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    e, r = np.asarray(e), np.asarray(r)
    n, D = len(e), ent.shape[1]
    L = D - TAPS + 1
    F = CH * L
    if m is None:
        m = masks(n, D, (0, 0, 0))
    m0, m1, m2 = (np.asarray(x, dtype=dtype) for x in m)
    assert T["fc.weight"].shape == (D, F), (T["fc.weight"].shape, D, F)
    img = ent[e]                                                              # [n, D]
    s = dict(img=img, n=n)
    stats = {}
    w0, b0 = T["bn0.weight"][0], T["bn0.bias"][0]
    if train:
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        y0, s["xh0"], mean, var, s["rstd0"], cnt = _bn(img, (0, 1), w0, b0, dtype)
        stats["bn0"] = (mean.reshape(1), var.reshape(1) * dtype(cnt) / dtype(cnt - 1))
    else:
        y0 = _bn_eval(img, T["bn0.running_mean"][0], T["bn0.running_var"][0], w0, b0, dtype)
    y0d = y0 * m0
    filt = (rel[r] @ T["fc1.weight"].T + T["fc1.bias"]).reshape(n, CH, TAPS)
    patches = np.stack([y0d[:, w:w + L] for w in range(TAPS)], 1)             # [n, 9, L]
    c = np.einsum("ncw,nwp->ncp", filt, patches)                              # [n, 32, L]
    if u_flip is not None:
        c = (c * (1 + np.random.default_rng(7919 + u_flip).choice([-1.0, 0.0, 1.0], size=c.shape) * 2.0 ** -24)).astype(dtype)
    w1, b1 = T["bn1.weight"][None, :, None], T["bn1.bias"][None, :, None]
    if train:
        y1, s["xh1"], mean, var, s["rstd1"], cnt = _bn(c, (0, 2), w1, b1, dtype)
        stats["bn1"] = (mean.reshape(CH), var.reshape(CH) * dtype(cnt) / dtype(cnt - 1))
    else:
        y1 = _bn_eval(c, T["bn1.running_mean"][None, :, None], T["bn1.running_var"][None, :, None], w1, b1, dtype)
    A = (y1 * m1[:, :, None]).reshape(n, F)
    if fc_order is not None:
        A = A[:, fc_order]
    u = A @ T["fc.weight"].T + T["fc.bias"]
    if u_flip is not None:
        u = (u * (1 + np.random.default_rng(u_flip).choice([-1.0, 0.0, 1.0], size=u.shape) * 2.0 ** -24)).astype(dtype)
    s.update(patches=patches, filt=filt, A=A, u=u, m=(m0, m1, m2), L=L, fc_order=fc_order)
    if train:
        y2, s["xh2"], mean, var, s["rstd2"], cnt = _bn(u * m2, (0,), T["bn2.weight"], T["bn2.bias"], dtype)
        stats["bn2"] = (mean.reshape(D), var.reshape(D) * dtype(n) / dtype(n - 1))
    else:
        y2 = _bn_eval(u, T["bn2.running_mean"], T["bn2.running_var"], T["bn2.weight"], T["bn2.bias"], dtype)   # bn2 in the eval form too
    s["y2"] = y2
    return np.maximum(y2, 0), s, stats


def body_backward(P, e, r, s, dx, dtype=np.float64):
    """The 13 gradients of one direction's training-form body given dx (b: zero, it is the head's; the lookup rows of id 0 dropped),
    and the cancellation scale (sum of the absolute summands) of the gradients that can vanish."""
    T = {key: np.asarray(P[key], dtype=dtype) for key in TENSORS}
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    e, r = np.asarray(e), np.asarray(r)
    n, D, L = s["n"], ent.shape[1], s["L"]
    m0, m1, m2 = s["m"]
    g, scale = {}, {}

    def bn_back(dy, xh, w, rstd, axes):
        cnt = dtype(np.prod([dy.shape[a] for a in axes]))
        S1, S2 = dy.sum(axis=axes, keepdims=True), (dy * xh).sum(axis=axes, keepdims=True)
        return w * rstd * (dy - S1 / cnt - xh * (S2 / cnt)), S1, S2

    dy2 = dx * (s["y2"] > 0)
    dud, S1, S2 = bn_back(dy2, s["xh2"], T["bn2.weight"], s["rstd2"], (0,))
    g["bn2.weight"], g["bn2.bias"] = S2.reshape(D), S1.reshape(D)
    du = dud * m2
    # (du is itself a difference of three terms, and with two rows it cancels altogether: the cancellation scale of what is summed from
    # it is built from the absolute values of those terms, not from |du|)
    du_abs = np.abs(T["bn2.weight"] * s["rstd2"]) * (np.abs(dy2) + np.abs(S1) / dtype(n) + np.abs(s["xh2"]) * (np.abs(S2) / dtype(n))) * m2
    g["fc.bias"], scale["fc.bias"] = du.sum(0), du_abs.sum(0).max()
    g["fc.weight"] = du.T @ s["A"]
    dA = du @ T["fc.weight"]
    if s.get("fc_order") is not None:
        dA = dA[:, np.argsort(s["fc_order"])]
    dy1 = dA.reshape(n, CH, L) * m1[:, :, None]
    dc, S1, S2 = bn_back(dy1, s["xh1"], T["bn1.weight"][None, :, None], s["rstd1"], (0, 2))
    g["bn1.weight"], g["bn1.bias"] = S2.reshape(CH), S1.reshape(CH)
    scale["bn1.bias"] = ((du_abs @ np.abs(T["fc.weight"])).reshape(n, CH, L) * m1[:, :, None]).sum((0, 2)).max()
    dfilt = np.einsum("ncp,nwp->ncw", dc, s["patches"]).reshape(n, CH * TAPS)
    g["fc1.bias"] = dfilt.sum(0)
    g["fc1.weight"] = dfilt.T @ rel[r]
    drel = dfilt @ T["fc1.weight"]
    dy0d = np.zeros((n, D), dtype=dtype)
    for w in range(TAPS):
        dy0d[:, w:w + L] += np.einsum("ncp,nc->np", dc, s["filt"][:, :, w])
    dy0 = dy0d * m0
    dent, S1, S2 = bn_back(dy0, s["xh0"], T["bn0.weight"][0], s["rstd0"], (0, 1))
    g["bn0.weight"], g["bn0.bias"] = S2.reshape(1), S1.reshape(1)
    scale["bn0.weight"] = np.abs(dy0 * s["xh0"]).sum()
    g["ent_embeddings.weight"], g["rel_embeddings.weight"] = np.zeros_like(ent), np.zeros_like(rel)
    np.add.at(g["ent_embeddings.weight"], e[e != 0], dent[e != 0])            # padding_idx = 0: the lookup's gradient of id 0 is dropped
    np.add.at(g["rel_embeddings.weight"], r[r != 0], drel[r != 0])
    g["b"] = np.zeros_like(T["b"])
    return g, {key: float(v) for key, v in scale.items()}


def update_buffers(buffers, stats, dtype=np.float64):
    """running = (1 - momentum) running + momentum (mean, unbiased variance), in place on the dict of running buffers."""
    for bn, (mean, var) in stats.items():
        buffers[bn + ".running_mean"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_mean"] + dtype(MOMENTUM) * mean
        buffers[bn + ".running_var"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_var"] + dtype(MOMENTUM) * var


def forward(P, e, r, direction="tail", m=None, train=False, dtype=np.float64):
    """[n, E] predictions of HypER.forward (no buffer update).  `direction` selects nothing: there is one relation table."""
    assert direction in ("head", "tail")
    x, _, _ = body(P, e, r, m, train, dtype)
    return sigmoid(x @ np.asarray(P["ent_embeddings.weight"], dtype=dtype).T + np.asarray(P["b"], dtype=dtype))


def step(P, h, r, t, y_hr_t, y_tr_h, dropouts=(0.0, 0.0, 0.0), seed=0, offset=0, label_smoothing=None, dtype=np.float64, mask_list=None,
         fc_order=None, u_flip=None):
    """One train_step_projection: dict(loss, grads, pred_tails, pred_heads, buffers (after the step: updated tail first, then head),
    scale (cancellation scales of the gradients that can vanish), margin (smallest |pre-ReLU value| of bn2's outputs), head_ent0 (the
    head's share of grad(ent)[0], which is all of it)).  y_*: dense multi-hot label rows [B, E].  mask_list: ((m0, m1, m2) of the tail
    direction, of the head direction) instead of the Philox masks."""
    ent = np.asarray(P["ent_embeddings.weight"], dtype=dtype)
    bias = np.asarray(P["b"], dtype=dtype)
    E, D = ent.shape
    B = len(h)
    buffers = {key: np.asarray(P[key], dtype=dtype).copy() for key in BUFFERS}
    grads = {key: np.zeros_like(np.asarray(P[key], dtype=dtype)) for key in TENSORS}
    scale = {key: 0.0 for key in ("bn0.weight", "fc.bias", "bn1.bias")}
    loss, preds, margin = dtype(0), [], np.inf
    head_ent0 = np.zeros(D, dtype=dtype)
    for side, (ee, yy) in enumerate(((h, y_hr_t), (t, y_tr_h))):
        m = mask_list[side] if mask_list is not None else masks(B, D, dropouts, seed, offset, row0=side * B)
        x, s, stats = body(P, ee, r, m, True, dtype, fc_order, None if u_flip is None else 2 * u_flip + side)
        update_buffers(buffers, stats, dtype)
        margin = min(margin, np.abs(s["y2"]).min())
        p = sigmoid(x @ ent.T + bias)
        Y = np.asarray(yy, dtype=dtype)
        if label_smoothing is not None:
            Y = Y * dtype(1.0 - label_smoothing) + dtype(1.0 / E)
        # BCEWithLogits applied to the sigmoid outputs (sic): softplus(p) - y p, mean over B * E per direction, the two added
        loss = loss + (np.log1p(np.exp(p)) - Y * p).sum() / dtype(B * E)
        dlogit = (sigmoid(p) - Y) / dtype(B * E) * p * (1 - p)
        dx = dlogit @ ent
        if u_flip is not None:     # (the head's sum over the entities is a rounded sum too)
            dx = (dx * (1 + np.random.default_rng(104729 + 2 * u_flip + side).choice([-1.0, 0.0, 1.0], size=dx.shape) * 2.0 ** -24)).astype(dtype)
        g, sc = body_backward(P, ee, r, s, dx, dtype)
        for key in TENSORS:
            grads[key] = grads[key] + g[key]
        head = dlogit.T @ x
        grads["ent_embeddings.weight"] = grads["ent_embeddings.weight"] + head
        head_ent0 = head_ent0 + head[0]
        grads["b"] = grads["b"] + dlogit.sum(0)
        for key in scale:
            scale[key] += sc[key]
        preds.append(p)
    return dict(loss=float(loss), grads=grads, pred_tails=preds[0], pred_heads=preds[1], buffers=buffers, scale=scale, margin=float(margin),
                head_ent0=head_ent0)


def eval_margin(P, test):
    """Smallest |pre-ReLU value| of bn2's outputs in the eval form over both sides of the test triples."""
    test = np.asarray(test)
    out = np.inf
    for ee in (test[:, 0], test[:, 2]):
        _, s, _ = body(P, ee, test[:, 1], None, False)
        out = min(out, np.abs(s["y2"]).min())
    return float(out)


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


def adam_trajectory(P, batches, lr, dropouts, seed, label_smoothing, dtype=np.float64, optimizer="adam", u_flip=None):
    """`len(batches)` Adam steps (torch defaults: betas 0.9 / 0.999, eps 1e-8; optimizer="sgd": plain SGD steps instead) of the fused step
    with the Philox masks of (seed, step):
    (per-step losses, final P with the running buffers, smallest pre-ReLU margin over the steps)."""
    P = {key: np.asarray(v, dtype=dtype).copy() for key, v in P.items() if key in TENSORS + BUFFERS}
    m1 = {key: np.zeros_like(P[key]) for key in TENSORS}
    m2 = {key: np.zeros_like(P[key]) for key in TENSORS}
    losses, margin = [], np.inf
    for i, (h, r, t, y1, y2) in enumerate(batches):
        out = step(P, h, r, t, y1, y2, dropouts=dropouts, seed=seed, offset=i, label_smoothing=label_smoothing, dtype=dtype,
                   u_flip=None if u_flip is None else 16 * u_flip + i)
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
