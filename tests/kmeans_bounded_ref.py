"""Plain numpy companions of the bounded k-means tests on top of tests/kmeans_ref.py: the runner-up distance by direct
differences and the one hard input, on which Lloyd's loop runs 20 iterations and every iteration after the first has both skipped
and active rows."""
import numpy as np

import kmeans_ref as kr

HARD = (1283, 33, 12)


def second(X, C, labels):
    """second[i] = the smallest directly differenced squared distance over the centroids other than labels[i]; +inf at k = 1, NaN
    where the label is -1."""
    D = kr.dists(X, C)
    D[np.arange(X.shape[0]), np.maximum(labels, 0)] = np.inf
    return np.where(labels < 0, np.nan, np.where(np.isnan(D), np.inf, D).min(axis=1))


def hard():
    """-> (X, ids): overlapping clusters (noise 1.0) and twice as many centroids as clusters, started from 12 drawn rows."""
    from conftest import clustered
    n, d, k = HARD
    return 4.0 * clustered(n, d, nclust=6, noise=1.0, seed=79, normalise=False), np.random.default_rng(5).choice(n, k, replace=False)
