"""float64 numpy restatement of ConvKB as the reference executes it (models/pointwise.py:241-318): the affine form of the score and
the gradients of the pointwise-logistic step with respect to the trainable tensors.  Written from the
formulas, not from the kernels: tests hold both the frozen reference outputs and the HIP path to it.

    preds(h, r, t) = c0 + <A_h, ent[h]> + <A_r, rel[r]> + <A_t, ent[t]>
    W = sum_j (k - s_j + 1),  off_j = sum_{i<j} (k - s_i + 1)
    A_row[d] = sum_j sum_f sum_{c < s_j, 0 <= d-c <= k-s_j} conv_j.weight[f,0,row,c] * fc1.weight[0, f W + off_j + d - c]
    c0       = fc1.bias + sum_j sum_f conv_j.bias[f] * sum_p fc1.weight[0, f W + off_j + p]
"""
import numpy as np


def make_params(ent, rel, fc_w, fc_b, conv_w, conv_b):
    """conv_w: list of [F, 1, 3, s_j] arrays in conv_list order, conv_b: list of [F] arrays."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    conv_w = [f64(w).reshape(w.shape[0], 3, -1) for w in conv_w]
    return dict(ent=f64(ent), rel=f64(rel), fc_w=f64(fc_w).reshape(-1), fc_b=float(np.asarray(fc_b).reshape(-1)[0]), conv_w=conv_w,
                conv_b=[f64(b) for b in conv_b], widths=[w.shape[2] for w in conv_w], F=conv_w[0].shape[0], k=np.asarray(ent).shape[1])


def params_from_fixture(z, prefix="init."):
    n = sum(1 for key in z if key.startswith("conv.") and key.endswith(".weight"))
    return make_params(z[prefix + "ent_embeddings.weight"], z[prefix + "rel_embeddings.weight"], z[prefix + "fc1.weight"],
                       z[prefix + "fc1.bias"], [z["conv.%d.weight" % j] for j in range(n)], [z["conv.%d.bias" % j] for j in range(n)])


def layout(P):
    """(W, [off_j])"""
    offs, off = [], 0
    for s in P["widths"]:
        offs.append(off)
        off += P["k"] - s + 1
    return off, offs


def collapse64(P):
    """A [3, k] (rows h, r, t) and c0."""
    k, F = P["k"], P["F"]
    W, offs = layout(P)
    V = P["fc_w"].reshape(F, W)
    A = np.zeros((3, k))
    c0 = P["fc_b"]
    for w, b, s, off in zip(P["conv_w"], P["conv_b"], P["widths"], offs):
        cols = k - s + 1
        Vj = V[:, off:off + cols]
        for row in range(3):
            for c in range(s):
                A[row, c:c + cols] += w[:, row, c] @ Vj
        c0 += float(b @ Vj.sum(1))
    return A, c0


def preds64(P, h, r, t):
    A, c0 = collapse64(P)
    return c0 + P["ent"][h] @ A[0] + P["rel"][r] @ A[1] + P["ent"][t] @ A[2]


def conv_forward64(P, h, r, t):
    """The reference's forward executed literally (convolutions, concatenation, fc1): the check of the affine form itself."""
    k, F = P["k"], P["F"]
    x = np.stack([P["ent"][h], P["rel"][r], P["ent"][t]], 1)          # [b, 3, k]
    outs = []
    for w, b, s in zip(P["conv_w"], P["conv_b"], P["widths"]):
        cols = k - s + 1
        z = np.zeros((len(x), F, cols))
        for c in range(s):
            z += np.einsum("fr,brp->bfp", w[:, :, c], x[:, :, c:c + cols])
        outs.append(z + b[None, :, None])
    return np.concatenate(outs, 2).reshape(len(x), -1) @ P["fc_w"] + P["fc_b"]


def step64(P, h, r, t, y):
    """Trainer.train_step_pointwise: loss = mean(softplus(y * preds)) and its gradients {ent, rel, fc_w [F W], fc_b}."""
    k, F = P["k"], P["F"]
    W, offs = layout(P)
    A, c0 = collapse64(P)
    y = np.asarray(y, dtype=np.float64)
    x = y * (c0 + P["ent"][h] @ A[0] + P["rel"][r] @ A[1] + P["ent"][t] @ A[2])
    loss = float(np.mean(np.logaddexp(0.0, x)))
    g = y / (1.0 + np.exp(-x)) / len(x)
    g_ent, g_rel = np.zeros_like(P["ent"]), np.zeros_like(P["rel"])
    np.add.at(g_ent, h, g[:, None] * A[0])
    np.add.at(g_ent, t, g[:, None] * A[2])
    np.add.at(g_rel, r, g[:, None] * A[1])
    X = np.stack([g @ P["ent"][h], g @ P["rel"][r], g @ P["ent"][t]])   # [3, k]
    G = float(g.sum())
    g_fc = np.zeros((F, W))
    for w, b, s, off in zip(P["conv_w"], P["conv_b"], P["widths"], offs):
        cols = k - s + 1
        part = np.outer(b, np.full(cols, G))
        for row in range(3):
            for c in range(s):
                part += np.outer(w[:, row, c], X[row, c:c + cols])
        g_fc[:, off:off + cols] = part
    return loss, dict(ent=g_ent, rel=g_rel, fc_w=g_fc.reshape(-1), fc_b=G)


def rank64(row, true, known=()):
    """(rank, filtered rank): candidates strictly below the true one; the filtered rank leaves out the known ones."""
    less = row < row[true]
    keep = np.ones(len(row), dtype=bool)
    kn = np.asarray([e for e in known if e != true], dtype=np.int64)
    if kn.size:
        keep[kn] = False
    return int(less.sum()), int((less & keep).sum())
