"""The numpy reference of late-interaction search, imported by tests/test_maxsim_api.py, tests/test_gpu_maxsim.py
and tools/maxsim_bench.py: the per-group maxima of per-vector scores, then S13's "sum" fold (tests/fused_ref.py) over them."""
import numpy as np

import fused_ref


def group_max(S, labels_of_ids):
    """(labels [G] ascending, M [J, G]) from per-vector scores S [J, m] and the label of each of the m scored items: M[j, g] = the
    largest non-NaN S[j, i] over the items i of label g, +0.0 where that is a zero of either sign, NaN where every one is NaN."""
    S = np.asarray(S, dtype=np.float64)
    lab = np.asarray(labels_of_ids, dtype=np.int64)
    if S.ndim != 2 or lab.shape != (S.shape[1],):
        raise ValueError(f"S {S.shape} and labels {lab.shape} do not belong together")
    labels, dense = np.unique(lab, return_inverse=True)
    if lab.shape[0] == 0:
        return labels, np.empty((S.shape[0], 0))
    if np.all(dense[1:] >= dense[:-1]):     # the groups are contiguous already
        ordered, sorted_dense = S, dense
    else:
        order = np.argsort(dense, kind="stable")
        ordered, sorted_dense = S[:, order], dense[order]
    starts = np.flatnonzero(np.concatenate([[True], sorted_dense[1:] != sorted_dense[:-1]]))
    M = np.fmax.reduceat(ordered, starts, axis=1)   # fmax ignores a NaN beside a number: NaN only where every member is NaN
    M = M + 0.0                                     # -0.0 + 0.0 is +0.0: a maximum of zero is +0.0
    return labels, M


def maxsim(S, labels_of_ids, w, served=None):
    """(labels [G] ascending, F [G]): S13's sum fold of w[j] * M[j] over the served rows, ascending."""
    labels, M = group_max(S, labels_of_ids)
    return labels, fused_ref.fuse(M, w, "sum", served)


def top(labels, F, n):
    """The first n of (labels, F) by (F descending, label ascending), NaN left out: (labels, scores)."""
    labels = np.asarray(labels, dtype=np.int64)
    F = np.asarray(F, dtype=np.float64)
    keep = ~np.isnan(F)
    labels, F = labels[keep], F[keep]
    order = np.lexsort((labels, -F))[:n]
    return labels[order], F[order]
