"""The numpy reference of batched late-interaction search, imported by tests/test_maxsim_batch_api.py,
tests/test_gpu_maxsim_batch.py and tools/maxsim_batch_bench.py: the per-group maxima of the flattened per-vector scores
(tests/maxsim_ref.py), then the batched S13 "sum" fold (tests/fused_batch_ref.py) of every need over its own rows, then
tests/maxsim_ref.py's order.  No arithmetic of its own."""
import fused_batch_ref
import maxsim_ref


def maxsim_batch(S, labels_of_ids, offsets, weights, served=None):
    """(labels [G] ascending, F [B, G]) from the flattened per-vector scores S [sum J_b, m], the label of each of the m scored
    items, offsets [B + 1] and flattened weights [sum J_b]: row b is S13's sum fold of w[v] * M[v] over need b's served rows,
    ascending; a need with no served row gets a row of NaN."""
    labels, M = maxsim_ref.group_max(S, labels_of_ids)
    return labels, fused_batch_ref.fuse_batch(M, offsets, weights, "sum", served)


def top_batch(labels, F, n):
    """Per need the first n of (labels, F[b]) by (F descending, label ascending), NaN left out: a list of B (labels, scores)."""
    return [maxsim_ref.top(labels, row, n) for row in F]


default_weights = fused_batch_ref.default_weights
