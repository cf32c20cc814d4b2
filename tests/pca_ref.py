"""numpy float64 restatement of kge_pca_fit / kge_pca_transform's contract (include/kge_hip.h): rows without a non-finite entry, their
mean, the sample covariance with divisor max(count - 1, 1), numpy.linalg.eigh, descending order, the clamp at 0, the sign rule."""
import numpy as np


def pca_ref(X):
    """-> mean [dim], cov [dim, dim], eigenvalue [dim], components [dim, dim] (row c: the axis of eigenvalue[c]), count."""
    X = np.asarray(X, np.float64)
    Z = X[np.isfinite(X).all(1)]
    count, dim = len(Z), X.shape[1]
    mean = Z.sum(0) / count if count else np.zeros(dim)
    if count < 2:
        return mean, np.zeros((dim, dim)), np.zeros(dim), np.eye(dim), count
    cov = (Z - mean).T @ (Z - mean) / (count - 1)
    lam, vec = np.linalg.eigh(cov)
    W = vec[:, ::-1].T
    big = W[np.arange(dim), np.abs(W).argmax(1)]   # every row's component of largest magnitude, the lowest index on a tie
    return mean, cov, np.maximum(lam[::-1], 0.0), W * np.where(big < 0, -1.0, 1.0)[:, None], count


def transform_ref(X, mean, components, eigenvalue, n_components, whiten=False):
    # float64 [n, n_components]; NaN rows for rows with a non-finite entry, 0 for a whitened component without variance
    X = np.asarray(X, np.float64)
    bad = ~np.isfinite(X).all(1)
    Y = (np.where(bad[:, None], 0.0, X) - mean) @ components[:n_components].T
    if whiten:
        sd = np.sqrt(eigenvalue[:n_components])
        Y = np.where(sd > 0, Y / np.where(sd > 0, sd, 1.0), 0.0)
    Y[bad] = np.nan
    return Y
