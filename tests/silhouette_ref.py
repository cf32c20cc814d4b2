"""The contract of kge_silhouette (include/kge_hip.h) restated in numpy float64: an [n, n] distance block and a loop over clusters."""
import numpy as np


def silhouette_ref(X, label, k, metric="l2"):
    """-> (s, a, b float64 [n], neighbor int32 [n], count int32 [k], score float64, D float64 [n, n])."""
    X, label = np.asarray(X, np.float64), np.asarray(label).astype(np.int64).copy()
    n = len(X)
    label[np.isnan(X).any(1) | (label < 0) | (label >= k)] = -1
    valid = label >= 0
    Xz = np.where(valid[:, None], X, 0.0)
    G = Xz @ Xz.T
    if metric == "cosine":
        D = np.maximum(1.0 - G, 0.0)
    else:
        sq = np.diag(G)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * G, 0.0))
    np.fill_diagonal(D, 0.0)                      # d(i, i) is excluded by index
    count = np.bincount(label[valid], minlength=k).astype(np.int32)
    a, b, s = (np.full(n, np.nan) for _ in range(3))
    neighbor = np.full(n, -1, np.int32)
    mean = np.full((n, k), np.inf)
    for c in np.flatnonzero(count):
        S = D[:, label == c].sum(1)
        own = label == c
        a[own] = S[own] / (count[c] - 1) if count[c] > 1 else 0.0
        mean[~own, c] = S[~own] / count[c]
    for i in np.flatnonzero(valid):
        s[i] = 0.0
        if np.isfinite(mean[i]).any():
            neighbor[i] = int(np.argmin(mean[i]))   # the first of equal means: the lower id
            b[i] = mean[i, neighbor[i]]
            if count[label[i]] > 1 and max(a[i], b[i]) > 0:
                s[i] = (b[i] - a[i]) / max(a[i], b[i])
    score = s[valid].astype(np.float32).astype(np.float64).mean() if valid.any() else np.nan
    return s, a, b, neighbor, count, score, D
