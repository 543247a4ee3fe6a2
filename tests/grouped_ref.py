"""The numpy reference of grouped search, imported by tests/test_grouped_api.py, tests/test_gpu_grouped.py and
tools/grouped_bench.py: the route there was before -- all scores on the host, one lexsort, one pass in that order."""
import numpy as np


def _in_order(ids, labels, scores, order, step=4096):
    """(id, label, score) as Python values in the given order, a block at a time: a caller that stops early pays for no more."""
    for a in range(0, len(order), step):
        o = order[a:a + step]
        yield from zip(ids[o].tolist(), labels[o].tolist(), scores[o].tolist())


def grouped(ids, labels, scores, n_groups, per_group):
    """The S14 answer from scores[j] of item ids[j] with label labels[j]: list[(label, list[(index, score)])].  NaN scores are
    dropped; -0.0 ties with +0.0 (0.0 is added for the ORDER, the returned score keeps its bits); items by (score descending,
    index ascending); groups in the order of their first member, the first n_groups of them, per_group members each."""
    ids, labels, scores = np.asarray(ids, dtype=np.int64), np.asarray(labels, dtype=np.int64), np.asarray(scores, dtype=np.float64)
    keep = ~np.isnan(scores)
    ids, labels, scores = ids[keep], labels[keep], scores[keep]
    order = np.lexsort((ids, -(scores + 0.0)))
    out, at, full = [], {}, 0
    for i, l, s in _in_order(ids, labels, scores, order):
        if l not in at:
            if len(out) == n_groups:
                continue
            at[l] = len(out)
            out.append((l, []))
        if len(out[at[l]][1]) < per_group:
            out[at[l]][1].append((i, s))
            full += len(out[at[l]][1]) == per_group
            if full == n_groups:   # every group that can appear is complete
                break
    return out
