"""The numpy reference of fused multi-query search, imported by tests/test_fused_api.py, tests/test_gpu_fused.py
and tools/fused_bench.py.  Every product and every sum below is one IEEE fp64 operation on arrays: numpy rounds each once and
fuses nothing, so the loops reproduce the bits of the device's fold."""
import numpy as np


def fuse(S, w, mode, served=None):
    """F [M] from per-vector scores S [J, M] and weights w [J]: rows in ascending order, rows whose `served` entry is false
    left out.  sum: F = w[0] * S[0], then F = F + w[j] * S[j].  max: F = w[0] * S[0], then F = t where (t > F) | isnan(F), else F:
    the first largest term wins, a NaN never displaces a number, F is NaN only if every term is."""
    S = np.asarray(S, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if S.ndim != 2 or w.shape != (S.shape[0],):
        raise ValueError(f"S {S.shape} and w {w.shape} do not belong together")
    if mode not in ("sum", "max"):
        raise ValueError(f"unknown mode {mode!r}")
    rows = [j for j in range(S.shape[0]) if served is None or served[j]]
    if not rows:
        raise ValueError("no vector is served")
    F = w[rows[0]] * S[rows[0]]
    for j in rows[1:]:
        t = w[j] * S[j]
        if mode == "sum":
            F = F + t
        else:
            with np.errstate(invalid="ignore"):
                F = np.where((t > F) | np.isnan(F), t, F)
    return F


def top(ids, F, k):
    """The first k of (ids, F) by (F descending, id ascending): (ids, scores)."""
    ids = np.asarray(ids, dtype=np.int64)
    F = np.asarray(F, dtype=np.float64)
    order = np.lexsort((ids, -F))[:k]
    return ids[order], F[order]
