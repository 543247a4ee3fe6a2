"""The numpy reference of batched fused search, imported by tests/test_fused_batch_api.py,
tests/test_gpu_fused_batch.py and tools/fused_batch_bench.py: need b owns the rows offsets[b] .. offsets[b + 1] - 1 of the flattened
per-vector scores, and its fold is tests/fused_ref.py's over those rows alone."""
import numpy as np

import fused_ref


def fuse_batch(S, offsets, weights, mode, served=None):
    """F [B, M] from the flattened per-vector scores S [sum J_b, M], offsets [B + 1] and flattened weights [sum J_b]: row b is
    `fused_ref.fuse` over need b's rows, rows whose `served` entry is false left out.  A need with no served row gets a row
    of NaN."""
    S = np.asarray(S, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    offsets = [int(o) for o in offsets]
    if S.ndim != 2 or w.shape != (S.shape[0],) or offsets[0] != 0 or offsets[-1] != S.shape[0]:
        raise ValueError(f"S {S.shape}, w {w.shape} and offsets {offsets[0]} .. {offsets[-1]} do not belong together")
    F = np.empty((len(offsets) - 1, S.shape[1]), dtype=np.float64)
    for b in range(len(offsets) - 1):
        lo, hi = offsets[b], offsets[b + 1]
        if hi <= lo:
            raise ValueError(f"need {b} is empty")
        sv = None if served is None else [bool(x) for x in served[lo:hi]]
        if sv is not None and not any(sv):
            F[b] = np.nan
        else:
            F[b] = fused_ref.fuse(S[lo:hi], w[lo:hi], mode, sv)
    return F


def default_weights(offsets):
    """1/J_b for every vector of need b, flattened."""
    J = np.diff(np.asarray(offsets, dtype=np.int64))
    return np.repeat(1.0 / J, J)
