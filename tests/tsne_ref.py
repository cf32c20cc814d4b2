"""The contract of kge_tsne_* (include/kge_hip.h) restated in numpy float64, written from the formulas: the expected values of the
t-SNE tests and the backend of the CPU plumbing tests.  gradient_ref / descent_ref with dtype=np.float32 are the float32 yardstick
the device results are measured against: the same formulas, every array in float32, numpy's own (pairwise) summation order."""
import types

import numpy as np
import torch


def cond_p_ref(d2, count, perplexity, tol=1e-5, shift=True, steps=100):
    """p_{j|i} float64 [n, k] and beta [n] from squared distances d2 [n, k] of which the first count[i] of row i are live: the
    binary search of sklearn.manifold._utils._binary_search_perplexity (beta from 1, doubled or halved while a bound is open,
    bisected after, `steps` steps at most, stop at |H - log perplexity| <= tol).  shift: the row's smallest live squared
    distance is subtracted first (the library's one difference; without it an all-underflowing row gets sklearn's 1e-8 floor)."""
    d2 = np.asarray(d2, np.float64)
    n, k = d2.shape
    P = np.zeros((n, k))
    betas = np.ones(n)
    want = np.log(perplexity)
    for i in range(n):
        c = int(min(max(int(count[i]), 0), k))
        if c == 0:
            continue
        d = d2[i, :c] - (d2[i, :c].min() if shift else 0.0)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(steps):
            p = np.exp(-d * beta)
            s = p.sum()
            if s == 0.0:
                s = 1e-8
            p = p / s
            diff = np.log(s) + beta * (d * p).sum() - want
            if abs(diff) <= tol:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        P[i, :c], betas[i] = p, beta
    return P, betas


def joint_ref(ids, cond_p, count):
    """Dense float64 [n, n]: P_ij = (p_{j|i} + p_{i|j}) / (2 n) over the union of the two neighbour graphs, zero diagonal."""
    ids, cond_p = np.asarray(ids), np.asarray(cond_p, np.float64)
    n, k = ids.shape
    C = np.zeros((n, n))
    for i in range(n):
        for m in range(int(min(count[i], k))):
            j = int(ids[i, m])
            if j >= 0 and j != i:
                C[i, j] = cond_p[i, m]
    return (C + C.T) / (2.0 * n)


def csr_of(P):
    """(row_off int64 [n + 1], col int32 [nnz], val float32 [nnz]) of the nonzero off-diagonal entries of a dense P."""
    n = P.shape[0]
    mask = (P != 0) & ~np.eye(n, dtype=bool)
    row_off = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    i, j = np.nonzero(mask)
    return row_off, j.astype(np.int32), P[i, j].astype(np.float32)


def dense_of(row_off, col, val, n):
    """Dense float64 [n, n] of a CSR (entries of one place add up: a duplicate shows)."""
    P = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(np.asarray(row_off)))
    np.add.at(P, (rows, np.asarray(col, np.int64)), np.asarray(val, np.float64))
    return P


def gradient_ref(P, Y, exaggeration=1.0, dtype=np.float64):
    """(grad [n, 2], Z, KL): w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij,
    grad_i = 4 (sum_j exaggeration P_ij w_ij (y_i - y_j) - (1 / Z) sum_j w_ij^2 (y_i - y_j)),
    KL = sum_{P_ij > 0} P_ij log(P_ij Z / w_ij) with the unexaggerated P.  Every array in `dtype`; KL in float64 from them."""
    P, Y = np.asarray(P, dtype), np.asarray(Y, dtype)
    n = Y.shape[0]
    one, four = dtype(1), dtype(4)
    D = Y[:, None, :] - Y[None, :, :]
    W = one / (one + (D * D).sum(-1, dtype=dtype))
    W[np.arange(n), np.arange(n)] = 0
    Z = W.sum(dtype=dtype)
    attr = ((dtype(exaggeration) * P * W)[:, :, None] * D).sum(1, dtype=dtype)
    rep = ((W * W)[:, :, None] * D).sum(1, dtype=dtype) / Z
    grad = four * (attr - rep)
    m = P > 0
    KL = float((P[m].astype(np.float64) * np.log(P[m].astype(np.float64) * float(Z) / W[m].astype(np.float64))).sum())
    return grad, Z, KL


def descent_ref(P, Y, n_iter, exaggeration=1.0, momentum=0.8, learning_rate=200.0, update=None, gains=None, dtype=np.float64,
                record_every=0, it0=0):
    """(Y, update, gains, trace): n_iter iterations of sklearn's _gradient_descent step without its early stopping,
       inc = update * grad < 0; gains = inc ? gains + 0.2 : gains * 0.8; gains = max(gains, 0.01);
       update = momentum * update - learning_rate * (gains * grad); Y += update,
    in `dtype`.  trace: (KL, |grad|_2) of the Y that iteration `it` started from, for every (it + 1) % record_every == 0."""
    Y = np.array(Y, dtype)
    update = np.zeros_like(Y) if update is None else np.array(update, dtype)
    gains = np.ones_like(Y) if gains is None else np.array(gains, dtype)
    trace = []
    for it in range(it0, it0 + n_iter):
        grad, _, kl = gradient_ref(P, Y, exaggeration, dtype)
        if record_every > 0 and (it + 1) % record_every == 0:
            trace.append((kl, float(np.sqrt((grad.astype(np.float64) ** 2).sum()))))
        inc = update * grad < 0
        gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
        gains = np.maximum(gains, dtype(0.01))
        update = (dtype(momentum) * update - dtype(learning_rate) * (gains * grad)).astype(dtype)
        Y = (Y + update).astype(dtype)
    return Y, update, gains, np.asarray(trace, np.float64).reshape(-1, 2)


def clustered(n, d, clusters=6, seed=0, centre_scale=3.0):
    """(rows float32 [n, d], labels [n]): seeded Gaussian clusters, centres N(0, centre_scale^2), unit noise."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, centre_scale, (clusters, d))
    labels = np.arange(n) % clusters
    return (centres[labels] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32), labels


def neighbours_l2(X, k):
    """(ids int32 [n, k], dist float32 [n, k], count int32 [n]) of the k nearest other rows under L2, nearer first, lower id first
    among equals: kge_knn_rows's output for the rows' own table."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    D[np.arange(n), np.arange(n)] = np.inf
    ids = np.argsort(D, 1, kind="stable")[:, :k].astype(np.int32)
    return ids, np.take_along_axis(D, ids.astype(np.int64), 1), np.full(n, k, np.int32)


def dense_P(X, perplexity):
    """The dense float64 P of rows X at the library's neighbour count min(n - 1, floor(3 perplexity))."""
    n = X.shape[0]
    ids, dist, count = neighbours_l2(X, min(n - 1, int(3 * perplexity)))
    p, _ = cond_p_ref(dist.astype(np.float64) ** 2, count, perplexity)
    return joint_ref(ids, p.astype(np.float32), count)


class Backend(types.SimpleNamespace):
    """The t-SNE entry points of pykg2vec_amd.kernels over CPU tensors, from the functions above: what the plumbing tests inject
    (with the search of knn_ref).  Calls are recorded in `calls`."""

    def __init__(self, **base):
        super().__init__(**base)
        self.calls = []

    def tsne_affinities(self, ids, dist, count, perplexity):
        self.calls.append(("affinities", tuple(dist.shape), float(perplexity)))
        p, beta = cond_p_ref(dist.numpy().astype(np.float64) ** 2, count.numpy(), perplexity)
        return torch.from_numpy(p.astype(np.float32)), torch.from_numpy(beta.astype(np.float32))

    def tsne_joint(self, ids, cond_p, count):
        from pykg2vec_amd import kernels
        P = joint_ref(ids.numpy(), cond_p.numpy(), count.numpy())
        ro, col, val = csr_of(P)
        self.P = P
        return kernels.TsneCSR(torch.from_numpy(ro), torch.from_numpy(col), torch.from_numpy(val), P.shape[0])

    def tsne_run(self, csr, Y, n_iter, it0=0, exaggeration=1.0, momentum=0.8, learning_rate=200.0, record_every=0, update=None,
                 gains=None, trace=None):
        self.calls.append(("run", int(n_iter), int(it0), float(exaggeration), float(momentum), float(learning_rate), int(record_every)))
        if it0 == 0:
            self.init = Y.clone()
        P = dense_of(csr.row_off.numpy(), csr.col.numpy(), csr.val.numpy(), csr.n)
        y, u, g, tr = descent_ref(P, Y.numpy(), n_iter, exaggeration, momentum, learning_rate, None if update is None else update.numpy(),
                                  None if gains is None else gains.numpy(), np.float64, record_every, it0)
        Y.copy_(torch.from_numpy(y.astype(np.float32)))
        if update is not None:
            update.copy_(torch.from_numpy(u.astype(np.float32)))
            gains.copy_(torch.from_numpy(g.astype(np.float32)))
        if trace is None:
            trace = torch.full(((it0 + n_iter) // record_every if record_every > 0 else 0, 2), float("nan"), dtype=torch.float64)
        if len(tr):
            first = it0 // record_every      # the slot (it + 1) // record_every - 1 of the first recorded it >= it0
            trace[first:first + len(tr)] = torch.from_numpy(tr)
        return Y, trace
