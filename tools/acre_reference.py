"""Float64 numpy restatement of AcrE (models/projection.py:621-746) with train_step_projection (utils/trainer.py:159-174) and
Criterion.multi_class_bce: the body in both ways and in its training and eval forms, loss, every gradient, the running-buffer updates
and the ranks.  The dropout masks are the Philox masks csrc/kge_acre.hip documents, built on oracle/sampler_oracle.py:philox4x32_10
(through tools/tucker_reference.py:mask, the same counter layout):

    key = (seed & 0xffffffff, seed >> 32);  counter = (elem, row >> 2, site | (offset >> 32) << 2, offset & 0xffffffff);  word = row & 3
    site 0 (input dropout): elem = pixel in [0, 400), the entity half first;  site 1 (feature-map dropout): elem = channel in [0, C);
    site 2 (hidden dropout): elem = j in [0, 200);  row = row0 + position in the call: the step numbers the h rows 0 .. B-1, the t rows
    B .. 2B-1;  keep iff word >= floor(p * 2^32) with p the float32 rate; kept elements are scaled by the float32 value 1 / (1 - p)

G, the geometry: a dict with in_channels, way ("serial" / "parallel"), first_atrous, second_atrous, third_atrous, acre_bias.  hidden_size
is 200 and the image 20 x 20 by construction.  A convolution is a sum over its nine taps of the zero-padded, shifted input.  There is
ONE relation table of 2 R rows; neither embedding has a padding_idx: every id's lookup gradient is summed.

VANISHING, derived on paper (a gradient that is zero analytically, or zero up to a batch norm's eps, is compared on its cancellation
scale, the sum of the absolute values of its summands):
    fc.bias     without hidden dropout: bn2 subtracts the column mean of u * m2 = u, so a constant added to a column of u changes nothing.
    conv3.bias  in the serial way, at every rate: it adds a per-channel constant to c = conv3(z2) + res, and bn1 subtracts the channel
                mean before anything else sees c (the feature-map mask comes after bn1).  The gradient is the per-channel sum of bn1's
                backward, which is zero identically.  In the parallel way the conv biases pass through the gate, which turns a
                per-channel constant into b[ch] * (row sums of a block of W_gate): no constant over the positions, nothing vanishes;
                W_gate_e.bias is a per-POSITION constant shared by the channels, which bn1 (per channel) does not remove either.
    conv1.bias, conv2.bias   do NOT vanish: with ZERO padding a constant input channel gives a conv output that is smaller at the border.
    bn0.bias    does NOT vanish under zero padding, unlike InteractE's circular case: the constant reaches c through the residual (a
                per-channel constant, removed by bn1) AND through the convolutions, whose border outputs move by less than the interior's.
    bn0.weight  vanishes (up to bn1's eps) only when c is HOMOGENEOUS in y0, i.e. bn0.bias = 0 and no (or zero) convolution biases, in the
                serial way: then c is w0 times a fixed linear image of xh0 * m0, and bn1 divides the factor out.  Otherwise it does not.

`dtype` selects the arithmetic (np.float64: the restatement; np.float32: the plain fp32 run whose error sets the tests' tolerances).
`order`: None, or a seed; the fc features, the gate's 1600 inputs and the channels between the serial convolutions are then renumbered by
a seeded permutation (the same model), so that every fc / gate / conv contraction is summed in another order.
P: a dict with the model's state-dict keys (parameters and running buffers)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.tucker_reference import dense_labels, mask, rank64, sigmoid  # noqa: E402,F401

K, HW, SIDE = 200, 400, 20
BUFFERS = ("bn0.running_mean", "bn0.running_var", "bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")
COUNTERS = ("bn0.num_batches_tracked", "bn1.num_batches_tracked", "bn2.num_batches_tracked")
EPS, MOMENTUM = 1e-5, 0.1


def tensors(G):
    """The parameters' state-dict keys in order: a module's bare parameter (bias) comes first."""
    out = ["bias", "ent_embeddings.weight", "rel_embeddings.weight", "bn0.weight", "bn0.bias", "bn1.weight", "bn1.bias", "bn2.weight",
           "bn2.bias", "fc.weight", "fc.bias"]
    for i in (1, 2, 3):
        out.append("conv%d.weight" % i)
        if G["acre_bias"]:
            out.append("conv%d.bias" % i)
    if G["way"] != "serial":
        out += ["W_gate_e.weight", "W_gate_e.bias"]
    return tuple(out)


def shapes(G, E, R):
    """{key: shape} of the parameters and the running buffers."""
    C = int(G["in_channels"])
    Cin = C if G["way"] == "serial" else 1
    s = {"bias": (E,), "ent_embeddings.weight": (E, K), "rel_embeddings.weight": (2 * R, K), "bn0.weight": (1,), "bn0.bias": (1,),
         "bn1.weight": (C,), "bn1.bias": (C,), "bn2.weight": (K,), "bn2.bias": (K,), "fc.weight": (K, HW * C), "fc.bias": (K,),
         "conv1.weight": (C, 1, 3, 3), "conv2.weight": (C, Cin, 3, 3), "conv3.weight": (C, Cin, 3, 3), "conv1.bias": (C,),
         "conv2.bias": (C,), "conv3.bias": (C,), "W_gate_e.weight": (HW, 4 * HW), "W_gate_e.bias": (HW,),
         "bn0.running_mean": (1,), "bn0.running_var": (1,), "bn1.running_mean": (C,), "bn1.running_var": (C,),
         "bn2.running_mean": (K,), "bn2.running_var": (K,)}
    return {key: s[key] for key in tensors(G) + BUFFERS}


LARGE = ("fc.weight", "W_gate_e.weight")   # too large to record whole: the fixtures hold a seed for the values, a sample of the gradient
N_SAMPLE = 4096


def gen_tensor(seed, scale, shape):
    """The fp32-exact values of a large tensor of a fixture: RandomState(seed).uniform(-1, 1) * scale rounded to fp32 (the stream of
    RandomState is frozen)."""
    return (np.random.RandomState(int(seed)).uniform(-1.0, 1.0, size=shape) * float(scale)).astype(np.float32)


def sample_index(seed, size):
    """The flat indices at which a fixture records a large gradient."""
    return np.random.RandomState(int(seed)).randint(0, size, size=N_SAMPLE)


def load_fixture(path):
    """(rec, G, P): the recorded arrays, the geometry, and the float64 state before the step with the large tensors regenerated."""
    z = np.load(path)
    rec = {key: z[key] for key in z.files}
    G = dict(in_channels=int(rec["in_channels"]), way=str(rec["way"]), first_atrous=int(rec["first_atrous"]),
             second_atrous=int(rec["second_atrous"]), third_atrous=int(rec["third_atrous"]), acre_bias=bool(rec["acre_bias"]))
    shp = shapes(G, int(rec["E"]), int(rec["R"]))
    for key in LARGE:
        if key in shp:
            rec[key] = gen_tensor(rec["gen." + key][0], rec["gen." + key][1], shp[key])
    P = {key: rec[key].astype(np.float64) for key in tensors(G) + BUFFERS}
    return rec, G, P


def dilations(G):
    return int(G["first_atrous"]), int(G["second_atrous"]), int(G["third_atrous"])


def vanishing(G, dropouts, P_=None):
    """The gradients that vanish analytically for this geometry at these rates (see the module docstring)."""
    out = []
    if not dropouts[2] > 0:
        out.append("fc.bias")
    if G["way"] == "serial":
        if G["acre_bias"]:
            out.append("conv3.bias")
        if P_ is not None and not np.any(np.asarray(P_["bn0.bias"])) and \
                not (G["acre_bias"] and any(np.any(np.asarray(P_["conv%d.bias" % i])) for i in (1, 2, 3))):
            out.append("bn0.weight")
    return tuple(out)


def masks(n, G, dropouts, seed=0, offset=0, row0=0, train=True):
    """(m0 [n, 20, 20], m1 [n, C], m2 [n, 200]) of the rows row0 .. row0 + n - 1."""
    if not train:
        dropouts = (0.0, 0.0, 0.0)
    m0, m1, m2 = (mask(site, row0 + n, elems, dropouts[site], seed, offset)[row0:]
                  for site, elems in ((0, HW), (1, int(G["in_channels"])), (2, K)))
    return m0.reshape(n, SIDE, SIDE), m1, m2


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


def _shift(x, dy, dx):
    """out[..., y, x] = x[..., y + dy, x + dx], zero outside the 20 x 20 image."""
    out = np.zeros_like(x)
    ys, yd = (slice(dy, SIDE), slice(0, SIDE - dy)) if dy >= 0 else (slice(0, SIDE + dy), slice(-dy, SIDE))
    xs, xd = (slice(dx, SIDE), slice(0, SIDE - dx)) if dx >= 0 else (slice(0, SIDE + dx), slice(-dx, SIDE))
    if abs(dy) < SIDE and abs(dx) < SIDE:
        out[..., yd, xd] = x[..., ys, xs]
    return out


def _taps(d):
    return [(3 * i + j, (i - 1) * d, (j - 1) * d) for i in range(3) for j in range(3)]


def conv(x, w, b, d):
    """The 3 x 3 cross-correlation with dilation d and zero padding d: x [n, Cin, 20, 20], w [Co, Cin, 3, 3] -> [n, Co, 20, 20]."""
    w9 = w.reshape(w.shape[0], w.shape[1], 9)
    out = np.zeros((x.shape[0], w.shape[0], SIDE, SIDE), dtype=x.dtype)
    for t, dy, dx in _taps(d):
        out += np.einsum("oi,nihw->nohw", w9[:, :, t], _shift(x, dy, dx))
    return out if b is None else out + b[None, :, None, None]


def conv_backward(x, w, d, dz):
    """(gw, gb, dx) of conv."""
    w9 = w.reshape(w.shape[0], w.shape[1], 9)
    gw = np.zeros_like(w9)
    dx_ = np.zeros_like(x)
    for t, dy, dx in _taps(d):
        gw[:, :, t] = np.einsum("nohw,nihw->oi", dz, _shift(x, dy, dx))
        dx_ += _shift(np.einsum("oi,nohw->nihw", w9[:, :, t], dz), -dy, -dx)
    return gw.reshape(w.shape), dz.sum((0, 2, 3)), dx_


def _orders(G, order):
    """(fc feature order, gate input order, channel order between the serial convolutions) or Nones."""
    if order is None:
        return None, None, None
    rs = np.random.RandomState(order)
    C = int(G["in_channels"])
    return rs.permutation(HW * C), rs.permutation(4 * HW), rs.permutation(C)


def body(P_, G, e, r, m=None, train=True, dtype=np.float64, order=None):
    """x [n, 200] of one direction, what the backward needs, and (training form) the batch statistics {bn: (mean, unbiased var)}."""
    T = {key: np.asarray(P_[key], dtype=dtype) for key in tensors(G) + BUFFERS}
    C, serial = int(G["in_channels"]), G["way"] == "serial"
    a = dilations(G)
    fo, go, co = _orders(G, order)
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    e, r = np.asarray(e), np.asarray(r)
    n = len(e)
    if m is None:
        m = masks(n, G, (0, 0, 0))
    m0, m1, m2 = (np.asarray(x, dtype=dtype) for x in m)
    m0 = m0.reshape(n, 1, SIDE, SIDE)
    assert T["fc.weight"].shape == (K, HW * C) and ent.shape[1] == K and rel.shape[1] == K
    img = np.concatenate([ent[e], rel[r]], 1).reshape(n, 1, SIDE, SIDE)
    s = dict(n=n)
    stats = {}
    w0, b0 = T["bn0.weight"][None, :, None, None], T["bn0.bias"][None, :, None, None]
    if train:
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        y0, s["xh0"], mean, var, s["rstd0"], cnt = _bn(img, (0, 2, 3), w0, b0, dtype)
        stats["bn0"] = (mean.reshape(1), var.reshape(1) * dtype(cnt) / dtype(cnt - 1))
    else:
        y0 = _bn_eval(img, T["bn0.running_mean"][None, :, None, None], T["bn0.running_var"][None, :, None, None], w0, b0, dtype)
    y0d = y0 * m0
    cw = [T["conv%d.weight" % i] for i in (1, 2, 3)]
    cb = [T.get("conv%d.bias" % i) if G["acre_bias"] else None for i in (1, 2, 3)]
    if serial:
        if co is not None:   # the channels of z1 and z2 renumbered: the same sums in another order
            inv = np.argsort(co)
            z1 = conv(y0d, cw[0][co], None if cb[0] is None else cb[0][co], a[0])
            z2 = conv(z1, cw[1][co][:, co], None if cb[1] is None else cb[1][co], a[1])
            z3 = conv(z2, cw[2][:, co], cb[2], a[2])
            z1, z2 = z1[:, inv], z2[:, inv]
        else:
            z1 = conv(y0d, cw[0], cb[0], a[0])
            z2 = conv(z1, cw[1], cb[1], a[1])
            z3 = conv(z2, cw[2], cb[2], a[2])
        c = z3 + y0d
        s.update(z1=z1, z2=z2)
    else:
        z = [conv(y0d, cw[i], cb[i], a[i]).reshape(n, C, HW) for i in range(3)]
        g_in = np.concatenate([np.broadcast_to(y0d.reshape(n, 1, HW), (n, C, HW))] + z, 2)   # [n, C, 1600]
        Wg = T["W_gate_e.weight"]
        c = ((g_in[:, :, go] @ Wg[:, go].T if go is not None else g_in @ Wg.T) + T["W_gate_e.bias"]).reshape(n, C, SIDE, SIDE)
        s.update(g_in=g_in)
    w1, b1 = T["bn1.weight"][None, :, None, None], T["bn1.bias"][None, :, None, None]
    if train:
        y1, s["xh1"], mean, var, s["rstd1"], cnt = _bn(c, (0, 2, 3), w1, b1, dtype)
        stats["bn1"] = (mean.reshape(C), var.reshape(C) * dtype(cnt) / dtype(cnt - 1))
    else:
        y1 = _bn_eval(c, T["bn1.running_mean"][None, :, None, None], T["bn1.running_var"][None, :, None, None], w1, b1, dtype)
    A = (np.maximum(y1, 0) * m1[:, :, None, None]).reshape(n, HW * C)
    u = (A[:, fo] @ T["fc.weight"][:, fo].T if fo is not None else A @ T["fc.weight"].T) + T["fc.bias"]
    s.update(y0d=y0d, A=A, u=u, y1=y1, m=(m0, m1, m2), order=order)
    if train:
        y2, s["xh2"], mean, var, s["rstd2"], cnt = _bn(u * m2, (0,), T["bn2.weight"], T["bn2.bias"], dtype)
        stats["bn2"] = (mean.reshape(K), var.reshape(K) * dtype(n) / dtype(n - 1))
    else:
        y2 = _bn_eval(u, T["bn2.running_mean"], T["bn2.running_var"], T["bn2.weight"], T["bn2.bias"], dtype)   # bn2 in the eval form too
    s["y2"] = y2
    return np.maximum(y2, 0), s, stats


def body_backward(P_, G, e, r, s, dx, dtype=np.float64):
    """The gradients of one direction's training-form body given dx (bias: zero, it is the head's), and the cancellation scale (sum of
    the absolute summands) of the gradients that can vanish."""
    T = {key: np.asarray(P_[key], dtype=dtype) for key in tensors(G)}
    C, serial = int(G["in_channels"]), G["way"] == "serial"
    a = dilations(G)
    fo, go, co = _orders(G, s.get("order"))
    ent, rel = T["ent_embeddings.weight"], T["rel_embeddings.weight"]
    e, r = np.asarray(e), np.asarray(r)
    n = s["n"]
    m0, m1, m2 = s["m"]
    g, scale = {}, {}

    def bn_back(dy, xh, w, rstd, axes):
        cnt = dtype(np.prod([dy.shape[a_] for a_ in axes]))
        S1, S2 = dy.sum(axis=axes, keepdims=True), (dy * xh).sum(axis=axes, keepdims=True)
        # (fourth value: the sum of the absolute values of the three terms, the cancellation scale of whatever is summed from the result)
        return (w * rstd * (dy - S1 / cnt - xh * (S2 / cnt)), S1, S2,
                np.abs(w * rstd) * (np.abs(dy) + np.abs(S1) / cnt + np.abs(xh) * (np.abs(S2) / cnt)))

    dy2 = dx * (s["y2"] > 0)
    dud, S1, S2, dud_abs = bn_back(dy2, s["xh2"], T["bn2.weight"], s["rstd2"], (0,))
    g["bn2.weight"], g["bn2.bias"] = S2.reshape(K), S1.reshape(K)
    du, du_abs = dud * m2, dud_abs * m2
    g["fc.bias"], scale["fc.bias"] = du.sum(0), du_abs.sum(0).max()
    if fo is not None:
        inv = np.argsort(fo)
        g["fc.weight"] = (du.T @ s["A"][:, fo])[:, inv]
        dA = (du @ T["fc.weight"][:, fo])[:, inv]
    else:
        g["fc.weight"] = du.T @ s["A"]
        dA = du @ T["fc.weight"]
    keep = m1[:, :, None, None] * (s["y1"] > 0)
    dy1 = dA.reshape(n, C, SIDE, SIDE) * keep
    dc, S1, S2, dc_abs = bn_back(dy1, s["xh1"], T["bn1.weight"][None, :, None, None], s["rstd1"], (0, 2, 3))
    g["bn1.weight"], g["bn1.bias"] = S2.reshape(C), S1.reshape(C)
    cw = [T["conv%d.weight" % i] for i in (1, 2, 3)]
    gb = [None, None, None]
    if serial:
        scale["conv3.bias"] = dc_abs.sum((0, 2, 3)).max()
        g["conv3.weight"], gb[2], dz2 = conv_backward(s["z2"], cw[2], a[2], dc)
        g["conv2.weight"], gb[1], dz1 = conv_backward(s["z1"], cw[1], a[1], dz2)
        g["conv1.weight"], gb[0], dy0d = conv_backward(s["y0d"], cw[0], a[0], dz1)
        dy0d = dy0d + dc.sum(1, keepdims=True)            # the residual, channels ascending
    else:
        dcf = dc.reshape(n, C, HW)
        Wg = T["W_gate_e.weight"]
        g["W_gate_e.weight"] = np.einsum("ncp,ncq->pq", dcf, s["g_in"])
        g["W_gate_e.bias"] = dcf.sum((0, 1))
        dg = dcf @ Wg                                      # [n, C, 1600]
        dy0d = dg[:, :, :HW].sum(1).reshape(n, 1, SIDE, SIDE)
        for i in range(3):
            g["conv%d.weight" % (i + 1)], gb[i], d_i = conv_backward(s["y0d"], cw[i], a[i],
                                                                     dg[:, :, HW * (i + 1):HW * (i + 2)].reshape(n, C, SIDE, SIDE))
            dy0d = dy0d + d_i
    if G["acre_bias"]:
        for i in range(3):
            g["conv%d.bias" % (i + 1)] = gb[i]
    dy0 = dy0d * m0
    dimg, S1, S2, _ = bn_back(dy0, s["xh0"], T["bn0.weight"][None, :, None, None], s["rstd0"], (0, 2, 3))
    g["bn0.weight"], g["bn0.bias"] = S2.reshape(1), S1.reshape(1)
    scale["bn0.weight"] = float((np.abs(dy0) * np.abs(s["xh0"])).sum())
    dcomb = dimg.reshape(n, 2 * K)
    g["ent_embeddings.weight"], g["rel_embeddings.weight"] = np.zeros_like(ent), np.zeros_like(rel)
    np.add.at(g["ent_embeddings.weight"], e, dcomb[:, :K])
    np.add.at(g["rel_embeddings.weight"], r, dcomb[:, K:])
    g["bias"] = np.zeros_like(T["bias"])
    return g, {key: float(v) for key, v in scale.items()}


def update_buffers(buffers, stats, dtype=np.float64):
    """running = (1 - momentum) running + momentum (mean, unbiased variance), in place on the dict of running buffers."""
    for bn, (mean, var) in stats.items():
        buffers[bn + ".running_mean"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_mean"] + dtype(MOMENTUM) * mean
        buffers[bn + ".running_var"] = dtype(1 - MOMENTUM) * buffers[bn + ".running_var"] + dtype(MOMENTUM) * var


def forward(P_, G, e, r, direction="tail", m=None, train=False, dtype=np.float64):
    """[n, E] predictions of AcrE.forward (no buffer update).  `direction` selects nothing: there is one relation table."""
    assert direction in ("head", "tail")
    x, _, _ = body(P_, G, e, r, m, train, dtype)
    return sigmoid(x @ np.asarray(P_["ent_embeddings.weight"], dtype=dtype).T + np.asarray(P_["bias"], dtype=dtype))


def step(P_, G, h, r, t, y_hr_t, y_tr_h, dropouts=(0.0, 0.0, 0.0), seed=0, offset=0, label_smoothing=None, dtype=np.float64, mask_list=None,
         order=None):
    """One train_step_projection: dict(loss, grads, pred_tails, pred_heads, buffers (after the step: updated tail first, then head),
    scale (cancellation scales of the gradients that can vanish), margin1 / margin2 (smallest |pre-ReLU value| of bn1's / bn2's outputs),
    margin (the smaller of the two)).  y_*: dense multi-hot label rows [B, E].  mask_list: ((m0, m1, m2) of the tail direction, of the
    head direction) instead of the Philox masks."""
    keys = tensors(G)
    ent = np.asarray(P_["ent_embeddings.weight"], dtype=dtype)
    bias = np.asarray(P_["bias"], dtype=dtype)
    E = ent.shape[0]
    B = len(h)
    buffers = {key: np.asarray(P_[key], dtype=dtype).copy() for key in BUFFERS}
    grads = {key: np.zeros_like(np.asarray(P_[key], dtype=dtype)) for key in keys}
    scale = {}
    loss, preds, margin1, margin2 = dtype(0), [], np.inf, np.inf
    for side, (ee, yy) in enumerate(((h, y_hr_t), (t, y_tr_h))):
        m = mask_list[side] if mask_list is not None else masks(B, G, dropouts, seed, offset, row0=side * B)
        x, s, stats = body(P_, G, ee, r, m, True, dtype, order)
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
        for key in keys:
            grads[key] = grads[key] + g[key]
        grads["ent_embeddings.weight"] = grads["ent_embeddings.weight"] + dlogit.T @ x
        grads["bias"] = grads["bias"] + dlogit.sum(0)
        for key in sc:
            scale[key] = scale.get(key, 0.0) + sc[key]
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


def trajectory(P_, G, batches, lr, dropouts, seed, label_smoothing, dtype=np.float64, optimizer="adam", order=None):
    """`len(batches)` Adam steps (torch defaults: betas 0.9 / 0.999, eps 1e-8; optimizer="sgd": plain SGD steps instead) of the fused step
    with the Philox masks of (seed, step): (per-step losses, final P with the running buffers, (smallest pre-ReLU margin of bn1's outputs,
    of bn2's outputs) over the steps)."""
    keys = tensors(G)
    P_ = {key: np.asarray(v, dtype=dtype).copy() for key, v in P_.items() if key in keys + BUFFERS}
    m1 = {key: np.zeros_like(P_[key]) for key in keys}
    m2 = {key: np.zeros_like(P_[key]) for key in keys}
    losses, margin = [], (np.inf, np.inf)
    for i, (h, r, t, y1, y2) in enumerate(batches):
        out = step(P_, G, h, r, t, y1, y2, dropouts=dropouts, seed=seed, offset=i, label_smoothing=label_smoothing, dtype=dtype, order=order)
        losses.append(out["loss"])
        margin = (min(margin[0], out["margin1"]), min(margin[1], out["margin2"]))
        P_.update(out["buffers"])
        for key in keys:
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
    return losses, P_, margin
