"""Float64 numpy restatement of InteractE (models/projection.py:347-505) with train_step_projection (utils/trainer.py:159-174) and
Criterion.multi_class_bce: the body in its training and eval forms, loss, the 12 gradients, the running-buffer updates and the ranks.
The dropout masks are the Philox masks csrc/kge_interacte.hip documents, built on oracle/sampler_oracle.py:philox4x32_10 (through
tools/tucker_reference.py:mask, the same counter layout):

    key = (seed & 0xffffffff, seed >> 32);  counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff);  word = row & 3
    site 0 (input dropout): elem = p H W + pixel in [0, 2k P);  site 1 (feature-map dropout): elem = channel in [0, P NF);  site 2
    (hidden dropout): elem = j in [0, k);  row = row0 + position in the call: the step numbers the h rows 0 .. B-1, the t rows B .. 2B-1
    keep iff word >= floor(p * 2^32) with p the float32 rate; kept elements are scaled by the float32 value 1 / (1 - p)

G, the geometry: a dict with reshape_height, reshape_width, feature_permutation, num_filters, kernel_size and chequer_perm [P, 2k]
(k = reshape_height * reshape_width; the image is H = 2 reshape_width high and W = reshape_height wide).  The circular convolution is
a sum of np.roll'ed images over the ks^2 taps.  Neither embedding has a padding_idx: every id's lookup gradient is summed.

VANISHING, derived on paper (a gradient that is zero analytically, or zero up to a batch norm's eps, is compared on its cancellation
scale, the sum of the absolute values of its summands):
    fc.bias     without hidden dropout: bn2 subtracts the column mean of u * m2 = u, so a constant added to a column of u changes nothing.
    bn0.bias    without input dropout: a constant b added to image p moves channel p NF + f of the CIRCULAR convolution by b * sum(taps of
                f) at every position -- with zero padding the border positions would move by less -- and bn1 subtracts the channel mean.
    bn0.weight  without input dropout: a factor on image p (on top of the constant above) is a factor on the centred conv output of
                its channels, which bn1 divides out again; the gradient survives through bn1's eps alone.  With input dropout the
                masked constant b0 * m0 is no constant and neither gradient vanishes (unless bn0.bias = 0, when bn0.weight still does).
    bn1.bias    does NOT vanish, unlike HypER's: a relu follows bn1 here, so a constant added to a channel reaches u only where the
                channel is positive, which is no constant per column of u.

`dtype` selects the arithmetic (np.float64: the restatement; np.float32: the plain fp32 run whose error sets the tests' tolerances).
P: a dict with the model's state-dict keys (parameters and running buffers)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.tucker_reference import dense_labels, mask, rank64, sigmoid  # noqa: E402,F401

TENSORS = ("bias", "conv_filt", "ent_embeddings.weight", "rel_embeddings.weight", "bn0.weight", "bn0.bias", "bn1.weight", "bn1.bias",
           "bn2.weight", "bn2.bias", "fc.weight", "fc.bias")   # state-dict order: a module's bare parameters come first
BUFFERS = ("bn0.running_mean", "bn0.running_var", "bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")
COUNTERS = ("bn0.num_batches_tracked", "bn1.num_batches_tracked", "bn2.num_batches_tracked")
EPS, MOMENTUM = 1e-5, 0.1


def geometry(G):
    """(k, H, W, P, NF, ks, pad, C, F, perm)."""
    rh, rw = int(G["reshape_height"]), int(G["reshape_width"])
    P, NF, ks = int(G["feature_permutation"]), int(G["num_filters"]), int(G["kernel_size"])
    k = rh * rw
    perm = np.asarray(G["chequer_perm"]).astype(np.int64).reshape(P, 2 * k)
    return k, 2 * rw, rh, P, NF, ks, ks // 2, P * NF, P * NF * 2 * k, perm


def chequer_perm(G, seed):
    """_get_chequer_perm of the reference after np.random.seed(seed): all entity permutations first, then all relation ones."""
    rh, rw, P = int(G["reshape_height"]), int(G["reshape_width"]), int(G["feature_permutation"])
    k = rh * rw
    np.random.seed(seed)
    ent_perm = [np.random.permutation(k) for _ in range(P)]
    rel_perm = [np.random.permutation(k) for _ in range(P)]
    out = np.zeros((P, 2 * k), dtype=np.int64)
    for p in range(P):
        idx = 0
        for i in range(rh):
            for _ in range(rw):
                pair = (ent_perm[p][idx], rel_perm[p][idx] + k)
                out[p, 2 * idx], out[p, 2 * idx + 1] = pair if (p + i) % 2 == 0 else pair[::-1]
                idx += 1
    return out


def vanishing(dropouts, bn0_bias=None):
    """The gradients that vanish analytically at these rates (see the module docstring)."""
    out = []
    if not dropouts[2] > 0:
        out.append("fc.bias")
    if not dropouts[0] > 0:
        out += ["bn0.bias", "bn0.weight"]
    elif bn0_bias is not None and not np.any(np.asarray(bn0_bias)):
        out.append("bn0.weight")
    return tuple(out)


VANISHING = vanishing


def masks(n, G, dropouts, seed=0, offset=0, row0=0, train=True):
    """(m0 [n, P, H, W], m1 [n, C], m2 [n, k]) of the rows row0 .. row0 + n - 1."""
    k, H, W, P, NF, ks, pad, C, F, perm = geometry(G)
    if not train:
        dropouts = (0.0, 0.0, 0.0)
    m0, m1, m2 = (mask(site, row0 + n, elems, dropouts[site], seed, offset)[row0:] for site, elems in ((0, 2 * k * P), (1, C), (2, k)))
    return m0.reshape(n, P, H, W), m1, m2


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


def _shifts(ks, pad):
    """(tap, roll shift) pairs: c += filt[:, tap] * roll(y0, shift), i.e. y0 read at (y + i - pad, x + j - pad) mod (H, W)."""
    return [(i * ks + j, (pad - i, pad - j)) for i in range(ks) for j in range(ks)]


def body(P_, G, e, r, m=None, train=True, dtype=np.float64, fc_order=None):
    """x [n, k] of one direction, what the backward needs, and (training form) the batch statistics {bn: (mean, unbiased var)}.
    fc_order: a permutation of the feature axis under which P["fc.weight"] is stored (the same model with its features renumbered: the
    tests use it to sum the fc product in another order)."""
    T = {key: np.asarray(P_[key], dtype=dtype) for key in TENSORS + BUFFERS}
    k, H, W, P, NF, ks, pad, C, F, perm = geometry(G)
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    e, r = np.asarray(e), np.asarray(r)
    n = len(e)
    if m is None:
        m = masks(n, G, (0, 0, 0))
    m0, m1, m2 = (np.asarray(x, dtype=dtype) for x in m)
    m0 = m0.reshape(n, P, H, W)
    assert T["fc.weight"].shape == (k, F), (T["fc.weight"].shape, k, F)
    filt = T["conv_filt"].reshape(NF, ks * ks)
    comb = np.concatenate([ent[e], rel[r]], 1)                                # [n, 2k]
    img = comb[:, perm].reshape(n, P, H, W)
    s = dict(n=n)
    stats = {}
    w0, b0 = T["bn0.weight"][None, :, None, None], T["bn0.bias"][None, :, None, None]
    if train:
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        y0, s["xh0"], mean, var, s["rstd0"], cnt = _bn(img, (0, 2, 3), w0, b0, dtype)
        stats["bn0"] = (mean.reshape(P), var.reshape(P) * dtype(cnt) / dtype(cnt - 1))
    else:
        y0 = _bn_eval(img, T["bn0.running_mean"][None, :, None, None], T["bn0.running_var"][None, :, None, None], w0, b0, dtype)
    y0d = y0 * m0
    rolled = np.stack([np.roll(y0d, sh, axis=(2, 3)) for _, sh in _shifts(ks, pad)], 0)   # [T, n, P, H, W]
    c = np.einsum("ft,tnphw->npfhw", filt, rolled).reshape(n, C, H, W)       # channel p NF + f
    w1, b1 = T["bn1.weight"][None, :, None, None], T["bn1.bias"][None, :, None, None]
    if train:
        y1, s["xh1"], mean, var, s["rstd1"], cnt = _bn(c, (0, 2, 3), w1, b1, dtype)
        stats["bn1"] = (mean.reshape(C), var.reshape(C) * dtype(cnt) / dtype(cnt - 1))
    else:
        y1 = _bn_eval(c, T["bn1.running_mean"][None, :, None, None], T["bn1.running_var"][None, :, None, None], w1, b1, dtype)
    A = (np.maximum(y1, 0) * m1[:, :, None, None]).reshape(n, F)
    if fc_order is not None:
        A = A[:, fc_order]
    u = A @ T["fc.weight"].T + T["fc.bias"]
    s.update(rolled=rolled, filt=filt, A=A, u=u, y1=y1, m=(m0, m1, m2), fc_order=fc_order)
    if train:
        y2, s["xh2"], mean, var, s["rstd2"], cnt = _bn(u * m2, (0,), T["bn2.weight"], T["bn2.bias"], dtype)
        stats["bn2"] = (mean.reshape(k), var.reshape(k) * dtype(n) / dtype(n - 1))
    else:
        y2 = _bn_eval(u, T["bn2.running_mean"], T["bn2.running_var"], T["bn2.weight"], T["bn2.bias"], dtype)   # bn2 in the eval form too
    s["y2"] = y2
    return np.maximum(y2, 0), s, stats


def body_backward(P_, G, e, r, s, dx, dtype=np.float64):
    """The 12 gradients of one direction's training-form body given dx (bias: zero, it is the head's), and the cancellation scale (sum of
    the absolute summands) of the gradients that can vanish."""
    T = {key: np.asarray(P_[key], dtype=dtype) for key in TENSORS}
    k, H, W, P, NF, ks, pad, C, F, perm = geometry(G)
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    e, r = np.asarray(e), np.asarray(r)
    n = s["n"]
    m0, m1, m2 = s["m"]
    g, scale = {}, {}

    def bn_back(dy, xh, w, rstd, axes):
        cnt = dtype(np.prod([dy.shape[a] for a in axes]))
        S1, S2 = dy.sum(axis=axes, keepdims=True), (dy * xh).sum(axis=axes, keepdims=True)
        # (second value: the sum of the absolute values of the three terms, the cancellation scale of whatever is summed from the result)
        return (w * rstd * (dy - S1 / cnt - xh * (S2 / cnt)), S1, S2,
                np.abs(w * rstd) * (np.abs(dy) + np.abs(S1) / cnt + np.abs(xh) * (np.abs(S2) / cnt)))

    dy2 = dx * (s["y2"] > 0)
    dud, S1, S2, dud_abs = bn_back(dy2, s["xh2"], T["bn2.weight"], s["rstd2"], (0,))
    g["bn2.weight"], g["bn2.bias"] = S2.reshape(k), S1.reshape(k)
    du, du_abs = dud * m2, dud_abs * m2
    g["fc.bias"], scale["fc.bias"] = du.sum(0), du_abs.sum(0).max()
    g["fc.weight"] = du.T @ s["A"]
    dA, dA_abs = du @ T["fc.weight"], du_abs @ np.abs(T["fc.weight"])
    if s.get("fc_order") is not None:
        inv = np.argsort(s["fc_order"])
        dA, dA_abs = dA[:, inv], dA_abs[:, inv]
    keep = m1[:, :, None, None] * (s["y1"] > 0)
    dy1, dy1_abs = dA.reshape(n, C, H, W) * keep, dA_abs.reshape(n, C, H, W) * keep
    dc, S1, S2, _ = bn_back(dy1, s["xh1"], T["bn1.weight"][None, :, None, None], s["rstd1"], (0, 2, 3))
    _, _, _, dc_abs = bn_back(dy1_abs, np.abs(s["xh1"]), np.abs(T["bn1.weight"])[None, :, None, None], s["rstd1"], (0, 2, 3))
    g["bn1.weight"], g["bn1.bias"] = S2.reshape(C), S1.reshape(C)
    dc5, dc5_abs = dc.reshape(n, P, NF, H, W), dc_abs.reshape(n, P, NF, H, W)
    g["conv_filt"] = np.einsum("npfhw,tnphw->ft", dc5, s["rolled"]).reshape(NF, 1, ks, ks)   # summed over the permutations: the shared filter
    dy0d, dy0d_abs = np.zeros((n, P, H, W), dtype=dtype), np.zeros((n, P, H, W), dtype=dtype)
    for t, sh in _shifts(ks, pad):
        dy0d += np.roll(np.einsum("npfhw,f->nphw", dc5, s["filt"][:, t]), (-sh[0], -sh[1]), axis=(2, 3))
        dy0d_abs += np.roll(np.einsum("npfhw,f->nphw", dc5_abs, np.abs(s["filt"][:, t])), (-sh[0], -sh[1]), axis=(2, 3))
    dy0, dy0_abs = dy0d * m0, dy0d_abs * m0
    dimg, S1, S2, _ = bn_back(dy0, s["xh0"], T["bn0.weight"][None, :, None, None], s["rstd0"], (0, 2, 3))
    g["bn0.weight"], g["bn0.bias"] = S2.reshape(P), S1.reshape(P)
    scale["bn0.bias"] = dy0_abs.sum((0, 2, 3)).max()
    scale["bn0.weight"] = (dy0_abs * np.abs(s["xh0"])).sum((0, 2, 3)).max()
    dcomb = np.zeros((n, 2 * k), dtype=dtype)
    for p in range(P):                                                        # ascending p, as the inverse gather sums
        dcomb[:, perm[p]] += dimg[:, p].reshape(n, 2 * k)
    g["ent_embeddings.weight"], g["rel_embeddings.weight"] = np.zeros_like(ent), np.zeros_like(rel)
    np.add.at(g["ent_embeddings.weight"], e, dcomb[:, :k])
    np.add.at(g["rel_embeddings.weight"], r, dcomb[:, k:])
    g["bias"] = np.zeros_like(T["bias"])
    return g, {key: float(v) for key, v in scale.items()}


def update_buffers(buffers, stats, dtype=np.float64):
    """running = (1 - momentum) running + momentum (mean, unbiased variance), in place on the dict of running buffers."""
    for bn, (mean, var) in stats.items():
        buffers[bn + ".running_mean"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_mean"] + dtype(MOMENTUM) * mean
        buffers[bn + ".running_var"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_var"] + dtype(MOMENTUM) * var


def forward(P_, G, e, r, direction="tail", m=None, train=False, dtype=np.float64):
    """[n, E] predictions of InteractE.forward (no buffer update).  `direction` selects nothing: there is one relation table."""
    assert direction in ("head", "tail")
    x, _, _ = body(P_, G, e, r, m, train, dtype)
    return sigmoid(x @ np.asarray(P_["ent_embeddings.weight"], dtype=dtype).T + np.asarray(P_["bias"], dtype=dtype))


def step(P_, G, h, r, t, y_hr_t, y_tr_h, dropouts=(0.0, 0.0, 0.0), seed=0, offset=0, label_smoothing=None, dtype=np.float64, mask_list=None,
         fc_order=None):
    """One train_step_projection: dict(loss, grads, pred_tails, pred_heads, buffers (after the step: updated tail first, then head),
    scale (cancellation scales of the gradients that can vanish), margin1 / margin2 (smallest |pre-ReLU value| of bn1's / bn2's outputs),
    margin (the smaller of the two)).
    y_*: dense multi-hot label rows [B, E].  mask_list: ((m0, m1, m2) of the tail direction, of the head direction) instead of the
    Philox masks."""
    ent = np.asarray(P_["ent_embeddings.weight"], dtype=dtype)
    bias = np.asarray(P_["bias"], dtype=dtype)
    E = ent.shape[0]
    B = len(h)
    buffers = {key: np.asarray(P_[key], dtype=dtype).copy() for key in BUFFERS}
    grads = {key: np.zeros_like(np.asarray(P_[key], dtype=dtype)) for key in TENSORS}
    scale = {key: 0.0 for key in ("bn0.weight", "bn0.bias", "fc.bias")}
    loss, preds, margin1, margin2 = dtype(0), [], np.inf, np.inf
    for side, (ee, yy) in enumerate(((h, y_hr_t), (t, y_tr_h))):
        m = mask_list[side] if mask_list is not None else masks(B, G, dropouts, seed, offset, row0=side * B)
        x, s, stats = body(P_, G, ee, r, m, True, dtype, fc_order)
        update_buffers(buffers, stats, dtype)
        margin1, margin2 = min(margin1, np.abs(s["y1"]).min()), min(margin2, np.abs(s["y2"]).min())
        p = sigmoid(x @ ent.T + bias)
        Y = np.asarray(yy, dtype=dtype)
        if label_smoothing is not None:
            Y = Y * dtype(1.0 - label_smoothing) + dtype(1.0 / E)
        # BCEWithLogits applied to the sigmoid outputs (sic): softplus(p) - y p, mean over B * E per direction, the two added
        loss = loss + (np.log1p(np.exp(p)) - Y * p).sum() / dtype(B * E)
        dlogit = (sigmoid(p) - Y) / dtype(B * E) * p * (1 - p)
        dx = dlogit @ ent
        g, sc = body_backward(P_, G, ee, r, s, dx, dtype)
        for key in TENSORS:
            grads[key] = grads[key] + g[key]
        grads["ent_embeddings.weight"] = grads["ent_embeddings.weight"] + dlogit.T @ x
        grads["bias"] = grads["bias"] + dlogit.sum(0)
        for key in scale:
            scale[key] += sc[key]
        preds.append(p)
    return dict(loss=float(loss), grads=grads, pred_tails=preds[0], pred_heads=preds[1], buffers=buffers, scale=scale, margin1=float(margin1),
                margin2=float(margin2), margin=float(min(margin1, margin2)))


def eval_margin(P_, G, test):
    """Smallest |pre-ReLU value| of bn1's and bn2's outputs in the eval form over both sides of the test triples."""
    test = np.asarray(test)
    out = np.inf
    for ee in (test[:, 0], test[:, 2]):
        _, s, _ = body(P_, G, ee, test[:, 1], None, False)
        out = min(out, np.abs(s["y2"]).min(), np.abs(s["y1"]).min())
    return float(out)


def ranks(P_, G, test, known):
    """int [4, n]: rank_head, rank_tail, filtered_rank_head, filtered_rank_tail (0-based) of the test triples in the eval form, float64,
    plus the smallest distance of another candidate's prediction to the true one's."""
    test = np.asarray(test)
    out = np.zeros((4, len(test)), dtype=np.int64)
    gap = np.inf
    pts = forward(P_, G, test[:, 0], test[:, 1], "tail")
    phs = forward(P_, G, test[:, 2], test[:, 1], "head")
    for i, (h, r, t) in enumerate(test):
        pt, ph = pts[i], phs[i]
        out[1, i], out[3, i] = rank64(pt, t, known[(known[:, 0] == h) & (known[:, 1] == r), 2])
        out[0, i], out[2, i] = rank64(ph, h, known[(known[:, 2] == t) & (known[:, 1] == r), 0])
        gap = min(gap, np.abs(np.delete(pt, t) - pt[t]).min(), np.abs(np.delete(ph, h) - ph[h]).min())
    return out, gap


def adam_trajectory(P_, G, batches, lr, dropouts, seed, label_smoothing, dtype=np.float64, optimizer="adam", fc_order=None):
    """`len(batches)` Adam steps (torch defaults: betas 0.9 / 0.999, eps 1e-8; optimizer="sgd": plain SGD steps instead) of the fused step
    with the Philox masks of (seed, step): (per-step losses, final P with the running buffers, smallest pre-ReLU margin over the steps).
    fc_order: the whole trajectory with the feature axis renumbered (fc.weight is permuted going in and coming out), i.e. with every fc
    sum taken in another order."""
    P_ = {key: np.asarray(v, dtype=dtype).copy() for key, v in P_.items() if key in TENSORS + BUFFERS}
    if fc_order is not None:
        P_["fc.weight"] = P_["fc.weight"][:, fc_order]
    m1 = {key: np.zeros_like(P_[key]) for key in TENSORS}
    m2 = {key: np.zeros_like(P_[key]) for key in TENSORS}
    losses, margin = [], np.inf
    for i, (h, r, t, y1, y2) in enumerate(batches):
        out = step(P_, G, h, r, t, y1, y2, dropouts=dropouts, seed=seed, offset=i, label_smoothing=label_smoothing, dtype=dtype,
                   fc_order=fc_order)
        losses.append(out["loss"])
        margin = min(margin, out["margin"])
        P_.update(out["buffers"])
        for key in TENSORS:
            g = out["grads"][key]
            if optimizer == "sgd":
                P_[key] = P_[key] - dtype(lr) * g
                continue
            # the optimiser's formulas as csrc/kge_opt_device.h states them (torch's _single_tensor_adam): the weights 1 - beta are
            # formed in the run's own precision (in fp32, 1 - 0.999 is 1.3e-5 off 0.001), the bias corrections in double
            m1[key] = m1[key] + (dtype(1) - dtype(0.9)) * (g - m1[key])
            m2[key] = m2[key] * dtype(0.999) + (dtype(1) - dtype(0.999)) * g * g
            denom = np.sqrt(m2[key]) / dtype(np.sqrt(1 - 0.999 ** (i + 1))) + dtype(1e-8)
            P_[key] = P_[key] - dtype(lr / (1 - 0.9 ** (i + 1))) * m1[key] / denom
    if fc_order is not None:
        P_["fc.weight"] = P_["fc.weight"][:, np.argsort(fc_order)]
    return losses, P_, margin
