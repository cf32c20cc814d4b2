"""numpy float64 restatement of kge_dbscan's contract (include/kge_hip.h): an [n, n] block of squared distances against eps^2 formed in
float64, counts, core flags, then a scan in row order that grows each cluster to completion (sklearn's dbscan_inner)."""
import numpy as np


def dbscan_ref(X, eps, min_samples, metric="l2"):
    """-> label int64 [n], core uint8 [n], count int32 [n], n_clusters, D [n, n] (what is compared) and the threshold it is compared
    with.  A row with a NaN is nobody's neighbour, not even its own; every other row is its own neighbour by index."""
    X = np.asarray(X, np.float64)
    n, bad = len(X), np.isnan(X).any(1)
    Z = np.where(bad[:, None], 0.0, X)
    if metric == "cosine":
        D, thr = np.maximum(1.0 - Z @ Z.T, 0.0), float(eps)
    else:
        D, thr = ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(2), float(eps) ** 2
    near = D <= thr
    near[np.arange(n), np.arange(n)] = True
    near[bad, :] = False
    near[:, bad] = False
    count = near.sum(1)
    core = count >= min_samples
    label, clusters = -np.ones(n, np.int64), 0
    for i in range(n):
        if label[i] != -1 or not core[i]:
            continue
        label[i], stack = clusters, [i]
        while stack:
            p = stack.pop()
            if core[p]:
                for q in np.flatnonzero(near[p] & (label == -1)):
                    label[q] = clusters
                    stack.append(q)
        clusters += 1
    return label, core.astype(np.uint8), count.astype(np.int32), clusters, D, thr
