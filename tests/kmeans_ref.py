"""The contract of kge_kmeans_* (include/kge_hip.h) restated in numpy, float64 where the contract says float64: the expected value of
the clustering tests."""
import numpy as np

CHUNK = 128   # KGE_KMEANS_CHUNK


def assign_ref(rows, centroids):
    """(label int32 [n], dist2 float64 [n], keys float64 [n, k]): the first centroid in the order (key, id) of the keys
    |c|^2 - 2 x.c, NaN keys last (-0.0 and +0.0 are one float64 value to argsort as well); a row with a NaN: label -1, dist2 NaN."""
    X, C = np.asarray(rows, np.float64), np.asarray(centroids, np.float64)
    with np.errstate(invalid="ignore"):
        keys = (C * C).sum(1)[None, :] - 2.0 * (X @ C.T)
    label = np.argmin(np.where(np.isnan(keys), np.inf, keys), 1).astype(np.int32)   # argmin: the lowest id among equal keys
    dist2 = ((X - C[label]) ** 2).sum(1)
    bad = np.isnan(X).any(1)
    label[bad] = -1
    dist2[bad] = np.nan
    return label, dist2, keys


def update_ref(rows, label, centroids, unit_centroids=False):
    """(centroids float32 [k, dim], count int32 [k]): members in ascending row id, chunks of CHUNK
    summed in float32 in member order, chunk sums added in float64 in chunk order, one rounding."""
    X, out = np.asarray(rows, np.float32), np.array(centroids, np.float32)
    count = np.zeros(len(out), np.int32)
    for c in range(len(out)):
        members, total = np.flatnonzero(np.asarray(label) == c), np.zeros(X.shape[1], np.float64)
        for a in range(0, len(members), CHUNK):
            s = np.zeros(X.shape[1], np.float32)
            for i in members[a:a + CHUNK]:
                s = s + X[i]
            total += s.astype(np.float64)
        if len(members) == 0:
            continue
        mean = total / len(members)
        if unit_centroids:
            norm = np.sqrt((mean * mean).sum())
            if not norm > 0:
                continue
            mean = mean / norm
        out[c], count[c] = mean.astype(np.float32), len(members)
    return out, count


def run_ref(rows, centroids, max_iter, unit_centroids=False, label=None, state=None):
    """(centroids, label, dist2, count, inertia, state) of kge_kmeans_run."""
    n = len(rows)
    C = np.array(centroids, np.float32)
    label = np.full(n, -2, np.int32) if label is None else np.array(label, np.int32)
    state = np.zeros(4, np.int32) if state is None else np.array(state, np.int32)
    dist2, count, inertia = np.full(n, np.nan), np.zeros(len(C), np.int32), np.nan
    for _ in range(max_iter):
        if state[0]:
            break
        new, dist2, _ = assign_ref(rows, C)
        changed = int((new != label).sum())
        label = new
        inertia = float(dist2[label >= 0].sum())
        C, count = update_ref(rows, label, C, unit_centroids)
        state = np.array([changed == 0, state[1] + 1, changed, (label < 0).sum()], np.int32)
    return C, label, dist2, count, inertia, state


def seed_ref(rows, k, u):
    """ids int32 [k] of kge_kmeans_seed: the first row without a NaN from floor(u[0] n) on, then the smallest i whose float64 prefix
    of d passes u[j] T; T not positive: the lowest row id not chosen yet."""
    X = np.asarray(rows, np.float64)
    n = len(X)
    bad = np.isnan(X).any(1)
    first = min(int(np.floor(u[0] * n)), n - 1)
    ids = [next((r % n for r in range(first, first + n) if not bad[r % n]), first)]
    d = np.full(n, np.inf)
    for j in range(1, k):
        with np.errstate(invalid="ignore"):
            new = ((X - X[ids[-1]]) ** 2).sum(1).astype(np.float32)
        d = np.where(bad, 0.0, np.where(new < d, new, d))
        P = np.cumsum(d.astype(np.float64))
        hit = np.flatnonzero(P > u[j] * P[-1])
        ids.append(int(hit[0]) if P[-1] > 0 and len(hit) else min(set(range(j + 1)) - set(ids)))
    return np.array(ids, np.int32)
