"""The numpy reference of late-interaction re-ranking of per-need candidate documents, imported by
tests/test_maxsim_lists_api.py, tests/test_gpu_maxsim_lists.py and tools/maxsim_lists_bench.py: per need, tests/maxsim_ref.py's
per-group maxima and S13 fold over that need's own rows of scores and its own entries.  No arithmetic of its own."""
import numpy as np

import maxsim_ref


def members(labels, wanted):
    """The items whose label is among `wanted`, ordered by (label ascending, item id ascending): the entries of a need whose
    candidate documents are `wanted` (any order, duplicates allowed)."""
    labels = np.asarray(labels, dtype=np.int64)
    idx = np.flatnonzero(np.isin(labels, np.asarray(wanted, dtype=np.int64)))
    return idx[np.lexsort((idx, labels[idx]))]


def maxsim_lists(S, labels_of_ids, weights, served=None):
    """A list of B (labels [G_b] ascending, F [G_b]) from, per need b, the scores S[b] [J_b, E_b] of its vectors over its entries,
    the label labels_of_ids[b] [E_b] of every entry, its weights weights[b] [J_b] and (optional) its served flags served[b]
    [J_b]: `maxsim_ref.maxsim` per need.  A need with no served row: every F is NaN."""
    out = []
    for b, (Sb, lab) in enumerate(zip(S, labels_of_ids)):
        Sb = np.asarray(Sb, dtype=np.float64)
        sv = None if served is None else list(served[b])
        if sv is not None and not any(sv):
            glab = np.unique(np.asarray(lab, dtype=np.int64))
            out.append((glab, np.full(len(glab), np.nan)))
            continue
        with np.errstate(all="ignore"):
            out.append(maxsim_ref.maxsim(Sb, lab, weights[b], sv))
    return out


def top_lists(per_need, n):
    """Per need the first n of (labels, F) by (F descending, label ascending), NaN left out: a list of B (labels, scores)."""
    return [maxsim_ref.top(lab, F, n) for lab, F in per_need]


def default_weights(Js):
    return [np.full(J, 1.0 / J) for J in Js]
