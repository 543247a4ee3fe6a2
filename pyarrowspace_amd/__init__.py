"""pyarrowspace_amd -- MI355X-native drop-in for the `arrowspace` Python module.

Host-side mirror of the reference's PyO3 surface (/root/reference/src/lib.rs:379-386):
`ArrowSpaceBuilder`, `ArrowSpace`, `GraphLaplacian`, `set_debug`.  Same names, same
argument order and meaning, same error behaviour; the arithmetic runs in hand-written
HIP kernels behind the C ABI of include/arrowspace_hip.h (libarrowspace_hip.so).
There is no CPU fallback: importing this package without the built library fails.
"""
from __future__ import annotations

import ctypes as C
import threading
import os

import numpy as np

from . import _lib
from ._lib import GraphParams, Opts

__all__ = ["ArrowSpaceBuilder", "ArrowSpace", "GraphLaplacian", "ItemSubset", "ItemGroups", "set_debug", "PanicException"]
__version__ = "0.1.0"

_L = _lib.load()


class PanicException(BaseException):
    """Mirror of pyo3_runtime.PanicException (a BaseException): raised where the
    reference panics, i.e. `assert_ne!(lambda_q, 0.0)` at src/lib.rs:156-159."""


def _raise(status: int):
    msg = _lib.last_error()
    if status == _lib.AS_EZEROLAMBDA:
        raise PanicException(msg or "The lambdas are zero, check the magnitude of items and eps.")
    if status in (_lib.AS_EINVAL, _lib.AS_EUNSUPPORTED):
        raise ValueError(msg)
    if status == _lib.AS_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def _check(status: int, stt=None, b: int = 0):
    """The end of every call into the library: its status, then (batched forms) the reference's panic for any of the b queries
    whose lambda_q is 0."""
    if status:
        _raise(status)
    if stt is not None:
        _panic_on_zero_lambda(stt, b)


def _panic_on_zero_lambda(stt, b: int):
    if (stt[:b] == _lib.AS_EZEROLAMBDA).any():
        raise PanicException("The lambdas are zero, check the magnitude of items and eps.")


def _need_gl(gl):
    if not isinstance(gl, GraphLaplacian):
        raise TypeError("argument 'gl': expected GraphLaplacian")


def _queries_2d(items) -> np.ndarray:
    Q = np.ascontiguousarray(items, dtype=np.float64)
    if Q.ndim != 2:
        raise TypeError("items must be a 2-D float64 array")
    return Q


def _handle(obj):
    return None if obj is None else obj._h


def _hit_buffers(count: int, kk: int):
    """Output buffers of `count` hit lists at stride kk (never empty: the C ABI wants pointers) and one status per query."""
    n = max(count * kk, 1)
    return np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64), np.zeros(max(count, 1), dtype=np.int64)


def _statuses(b: int) -> np.ndarray:
    return np.zeros(max(b, 1), dtype=np.int32)


def _hit_lists(idx, sc, ln, count: int, kk: int, per: int = 0):
    """The C ABI's hit lists: list p holds ln[p] (index, score) entries at stride kk.  per > 0: nested, `per` lists per query
    (a sweep; the caller answers an empty sweep itself)."""
    idx, sc = idx.reshape(-1)[:count * kk].reshape(count, kk).tolist(), sc.reshape(-1)[:count * kk].reshape(count, kk).tolist()
    # (tolist + zip: element-wise int()/float() over the arrays cost 1.5 ms per 256 queries, a fifth of the GPU time)
    flat = [list(zip(ii[:l], ss[:l])) for ii, ss, l in zip(idx, sc, ln.reshape(-1)[:count].tolist())]
    return [flat[i:i + per] for i in range(0, count, per)] if per else flat


def _counters(fn, handle, names) -> dict:
    out = (C.c_int64 * len(names))()
    _check(fn(handle, out, len(names)))
    return dict(zip(names, list(out)))


def set_debug(enabled: bool) -> None:
    """src/helpers.rs:12-14: process-global flag; messages go to stderr as `[pyarrowspace] ...`."""
    _L.as_set_debug(1 if enabled else 0)


if os.environ.get("ARROWSPACE_DEBUG", "") not in ("", "0"):
    set_debug(True)


def enable_search_stats(enabled: bool) -> None:
    """Extension: record HIP events around the scan kernel of every search (off by default)."""
    _L.as_enable_search_stats(1 if enabled else 0)


NORTH_STAR_MODE = {"metric": "l2", "kernel": "gaussian", "lambda_mode": "item"}        # BASELINE.json north_star
REFERENCE_MODE = {"metric": "cosine", "kernel": "rational", "lambda_mode": "item"}      # GRAPH_VARIABLES.md:7-10


def _parse_graph_params(graph_params, mode=None) -> tuple[GraphParams, Opts]:
    """src/helpers.rs:48-76.  eps,k,topk,p required; sigma missing/None -> eps*0.5.
    Keys the reference ignores select the documented variants: 'metric' in
    {'l2','cosine'}, 'kernel' in {'gaussian','rational'}, 'lambda_mode' in {'item','feature'}
    (DESIGN.md section 2).  Precedence: the dict's keys, then env ARROWSPACE_METRIC / _KERNEL / _LAMBDA_MODE, then
    `mode` -- the defaults of the module the caller imported (NORTH_STAR_MODE for pyarrowspace_amd and bench.py,
    REFERENCE_MODE for the reference-named module `arrowspace`, whose scripts' parameter sets are rectified-cosine
    distances)."""
    mode = NORTH_STAR_MODE if mode is None else mode
    gp, op = GraphParams(), Opts()
    op.device = int(os.environ.get("ARROWSPACE_DEVICE", "-1"))
    metric = os.environ.get("ARROWSPACE_METRIC", mode["metric"])
    kernel = os.environ.get("ARROWSPACE_KERNEL", mode["kernel"])
    lmode = os.environ.get("ARROWSPACE_LAMBDA_MODE", mode["lambda_mode"])
    if graph_params is None:
        # builder defaults (GRAPH_VARIABLES.md:15: eps~1e-3, k~6, p=2, sigma:=eps)
        gp.eps, gp.k, gp.topk, gp.p, gp.sigma, gp.has_sigma = 1e-3, 6, 3, 2.0, 1e-3, 1
    else:
        if not isinstance(graph_params, dict):
            raise TypeError("graph_params must be a dict or None")
        for key in ("eps", "k", "topk", "p"):
            if key not in graph_params:
                raise ValueError(f"graph_params['{key}'] is required")
        gp.eps = float(graph_params["eps"])
        for key in ("k", "topk"):
            v = graph_params[key]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise TypeError(f"graph_params['{key}'] must be a non-negative integer")
        gp.k, gp.topk = int(graph_params["k"]), int(graph_params["topk"])
        gp.p = float(graph_params["p"])
        sigma = graph_params.get("sigma", None)
        if sigma is None:
            gp.sigma, gp.has_sigma = 0.0, 0
        else:
            gp.sigma, gp.has_sigma = float(sigma), 1
        metric = graph_params.get("metric", metric)
        kernel = graph_params.get("kernel", kernel)
        lmode = graph_params.get("lambda_mode", lmode)
        op.force_exact = 1 if graph_params.get("force_exact", False) else 0
        op.keep_f64 = 1 if graph_params.get("keep_f64", False) else 0
        # test hook: start searches on a fallback path (bit0 fp64, bit1 wavefront-list selection)
        op.search_mode = int(graph_params.get("_search_mode", 0))
    if metric not in _lib.METRICS:
        raise ValueError(f"unknown metric {metric!r}; expected one of {sorted(_lib.METRICS)}")
    if kernel not in _lib.KERNELS:
        raise ValueError(f"unknown kernel {kernel!r}; expected one of {sorted(_lib.KERNELS)}")
    if lmode not in _lib.LAMBDA_MODES:
        raise ValueError(f"unknown lambda_mode {lmode!r}; expected one of {sorted(_lib.LAMBDA_MODES)}")
    op.metric, op.kernel, op.lambda_mode = _lib.METRICS[metric], _lib.KERNELS[kernel], _lib.LAMBDA_MODES[lmode]
    return gp, op


class GraphLaplacian:
    """Opaque handle of the normalised graph Laplacian (src/lib.rs:26-62)."""

    def __new__(cls, *a, **k):
        raise ValueError("GraphLaplacian cannot be constructed directly; use ArrowSpaceBuilder.build_with_graph")

    @classmethod
    def _wrap(cls, handle):
        self = object.__new__(cls)
        self._h = handle
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:      # _L is None once the interpreter tears the module down
            _L.as_free_graph(h)
            self._h = None

    @property
    def nnodes(self) -> int:
        return int(_L.as_nnodes(self._h))

    def shape(self) -> tuple[int, int]:
        n = self.nnodes
        return (n, n)

    @property
    def graph_params(self) -> dict:
        """src/lib.rs:49-61: dict {eps,k,topk,p,sigma} with sigma resolved."""
        gp = GraphParams()
        st = _L.as_get_graph_params(self._h, C.byref(gp))
        if st:
            _raise(st)
        return {"eps": gp.eps, "k": int(gp.k), "topk": int(gp.topk), "p": gp.p, "sigma": gp.sigma}

    # ---- extensions (no reference counterpart) ----
    @property
    def tau0(self) -> float:
        return float(_L.as_graph_tau0(self._h))

    @property
    def lambda_mode(self) -> str:
        """'item': N-node item graph, normalised Laplacian.  'feature': the F x F feature-space
        Laplacian L = D - W of TAUMODE.md:8,12-27 (nnodes == nfeatures)."""
        return "feature" if _L.as_graph_lambda_mode(self._h) == 1 else "item"

    def degrees(self) -> np.ndarray:
        out = np.empty(self.nnodes, dtype=np.float64)
        st = _L.as_graph_degrees(self._h, out.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        return out

    def to_csr(self):
        """(indptr, indices, values), columns ascending: L = I - D^-1/2 W D^-1/2 of the item graph, or
        L = D - W of the feature graph (lambda_mode 'feature')."""
        n, nnz = self.nnodes, int(_L.as_graph_nnz(self._h))
        indptr = np.empty(n + 1, dtype=np.int64)
        indices = np.empty(nnz, dtype=np.int64)
        values = np.empty(nnz, dtype=np.float64)
        st = _L.as_graph_csr(self._h, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                             values.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        return indptr, indices[: indptr[-1]], values[: indptr[-1]]

    def to_csr_dist(self):
        """Extension: (indptr, indices, dist) of the stored item graph as the device holds it: no diagonal, columns ascending,
        dist[e] the distance d_ij of entry e -- the structure of `to_csr()` with its diagonal removed.  The values
        `ArrowSpace.components(max_dist=...)` compares its threshold with.  A feature-mode graph raises ValueError."""
        n, nnz = self.nnodes, max(int(_L.as_graph_nnz(self._h)) - self.nnodes, 0)
        indptr = np.empty(n + 1, dtype=np.int64)
        indices = np.empty(max(nnz, 1), dtype=np.int64)
        dist = np.empty(max(nnz, 1), dtype=np.float64)
        st = _L.as_graph_csr_dist(self._h, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                                  dist.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        return indptr, indices[: indptr[-1]], dist[: indptr[-1]]

    def build_stats(self) -> dict:
        out = np.zeros(10, dtype=np.float64)
        _L.as_build_stats(self._h, out.ctypes.data_as(C.c_void_p), 10)
        keys = ("ingest_s", "knn_mfma_s", "refine_s", "fallback_s", "graph_s", "total_s", "fallback_rows", "mfma_flops",
                "unproven_rows", "band_rows")
        return dict(zip(keys, out.tolist()))


def _item_ids(ids_or_mask, nitems: int, what: str = "ids") -> np.ndarray:
    """Item ids as a contiguous int64 array: an integer array or sequence as it is (any order, duplicates kept), a boolean
    mask of length nitems through np.flatnonzero."""
    a = np.asarray(ids_or_mask)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != nitems:
            raise ValueError(f"argument '{what}': a boolean mask must have length nitems ({nitems}), got shape {a.shape}")
        return np.flatnonzero(a).astype(np.int64)
    if a.size == 0 and a.ndim == 1:
        return np.empty(0, dtype=np.int64)   # (numpy types an empty list float64: an empty selection has no ids to mistype)
    if a.dtype.kind not in "iu":
        raise TypeError(f"argument '{what}': expected integer item ids or a boolean mask, got dtype {a.dtype}")
    if a.ndim != 1:
        raise TypeError(f"argument '{what}': expected a 1-D sequence of item ids")
    if a.dtype == np.uint64 and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"argument '{what}': id {int(a.max())} is outside [0, {nitems})")
    return np.ascontiguousarray(a, dtype=np.int64)


def _min_scores(min_score, b: int) -> np.ndarray:
    """The thresholds of a range search as a contiguous float64 array of b entries: a number for every query, or a 1-D
    sequence of b numbers.  -inf and +inf are legal.  NaN, a wrong length or a wrong rank raise ValueError, anything that
    is not a number TypeError."""
    a = np.asarray(min_score)
    if a.dtype.kind not in "fiu":
        raise TypeError(f"argument 'min_score': expected a float or a sequence of floats, got dtype {a.dtype}")
    a = a.astype(np.float64)
    if a.ndim == 0:
        a = np.full(b, float(a), dtype=np.float64)
    elif a.ndim != 1:
        raise ValueError(f"argument 'min_score': expected a float or a 1-D sequence of {b} floats, got shape {a.shape}")
    elif a.shape[0] != b:
        raise ValueError(f"argument 'min_score': {a.shape[0]} thresholds for {b} queries")
    if np.isnan(a).any():
        raise ValueError("argument 'min_score': a threshold must not be NaN")
    return np.ascontiguousarray(a)


FUSED_MODES = {"sum": 0, "max": 1}


def _fused_args(items, gl, weights, mode, on_zero_lambda):
    """What the fused forms check before they touch a handle -> (Q float64 [J, D] contiguous, weights float64 [J] or None,
    mode number, skip flag).  TypeError: a `gl` that is no GraphLaplacian, items that are not 2-D, weights that are not numbers;
    ValueError: no vector at all, an unknown mode or on_zero_lambda, a weights length other than J (or a wrong rank), a NaN or
    infinite weight."""
    _need_gl(gl)
    Q = _queries_2d(items)
    if not isinstance(mode, str) or mode not in FUSED_MODES:
        raise ValueError(f"argument 'mode': expected 'sum' or 'max', got {mode!r}")
    if not isinstance(on_zero_lambda, str) or on_zero_lambda not in ("raise", "skip"):
        raise ValueError(f"argument 'on_zero_lambda': expected 'raise' or 'skip', got {on_zero_lambda!r}")
    j = Q.shape[0]
    if j < 1:
        raise ValueError("items must hold at least one query vector")
    w = None
    if weights is not None:
        w = np.asarray(weights)
        if w.dtype.kind not in "fiu":
            raise TypeError(f"argument 'weights': expected a sequence of floats, got dtype {w.dtype}")
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim != 1 or w.shape[0] != j:
            raise ValueError(f"argument 'weights': expected {j} weights, one per query vector, got shape {w.shape}")
        if not np.isfinite(w).all():
            raise ValueError("argument 'weights': a weight must be finite")
    return Q, w, FUSED_MODES[mode], 1 if on_zero_lambda == "skip" else 0


def _fused_batch_args(needs, gl, weights, mode, on_zero_lambda):
    """What the batched fused forms check before they touch a handle: `_fused_args`' checks, need by need, the message naming
    the need -> (V float64 [sum J_b, D] contiguous: the vectors flattened in need order, offsets int64 [B + 1], weights float64
    [sum J_b] or None (a need whose entry is None gets 1/J_b each), mode number, skip flag).  TypeError: a `gl` that is no
    GraphLaplacian, a need that is not 2-D, weights that are not numbers; ValueError: no needs, an empty need, a wrong weight
    count, a NaN or infinite weight, needs of differing D, an unknown mode or on_zero_lambda."""
    _need_gl(gl)
    if not isinstance(mode, str) or mode not in FUSED_MODES:
        raise ValueError(f"argument 'mode': expected 'sum' or 'max', got {mode!r}")
    if not isinstance(on_zero_lambda, str) or on_zero_lambda not in ("raise", "skip"):
        raise ValueError(f"argument 'on_zero_lambda': expected 'raise' or 'skip', got {on_zero_lambda!r}")
    if isinstance(needs, np.ndarray) and needs.ndim != 3:
        raise TypeError(f"argument 'needs': expected a 3-D array (B, J, D) or a sequence of B 2-D arrays, got shape {needs.shape}")
    if isinstance(needs, (str, bytes)) or not hasattr(needs, "__iter__"):
        raise TypeError("argument 'needs': expected a 3-D array (B, J, D) or a sequence of B 2-D arrays")
    seq = list(needs)
    if not seq:
        raise ValueError("needs must hold at least one need")
    mats = []
    for b, need in enumerate(seq):
        try:
            Q = np.ascontiguousarray(need, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"need {b} must be a 2-D float64 array") from None
        if Q.ndim != 2:
            raise TypeError(f"need {b} must be a 2-D float64 array, got shape {Q.shape}")
        if Q.shape[0] < 1:
            raise ValueError(f"need {b} must hold at least one query vector")
        if mats and Q.shape[1] != mats[0].shape[1]:
            raise ValueError(f"need {b} has D = {Q.shape[1]}, need 0 has D = {mats[0].shape[1]}: every need must have the same D")
        mats.append(Q)
    offs = np.zeros(len(mats) + 1, dtype=np.int64)
    np.cumsum([Q.shape[0] for Q in mats], out=offs[1:])
    w = None
    if weights is not None:
        if isinstance(weights, (str, bytes)):
            raise TypeError("argument 'weights': expected one sequence of floats per need")
        if not hasattr(weights, "__iter__"):
            raise ValueError(f"argument 'weights': expected {len(mats)} entries, one per need, got {weights!r}")
        wl = list(weights)
        if len(wl) != len(mats):
            raise ValueError(f"argument 'weights': expected {len(mats)} entries, one per need, got {len(wl)}")
        parts = []
        for b, (Q, wb) in enumerate(zip(mats, wl)):
            j = Q.shape[0]
            if wb is None:
                parts.append(np.full(j, 1.0 / j))
                continue
            wb = np.asarray(wb)
            if wb.dtype.kind not in "fiu":
                raise TypeError(f"argument 'weights': need {b}: expected a sequence of floats, got dtype {wb.dtype}")
            wb = np.ascontiguousarray(wb, dtype=np.float64)
            if wb.ndim != 1 or wb.shape[0] != j:
                raise ValueError(f"argument 'weights': need {b}: expected {j} weights, one per query vector, got shape {wb.shape}")
            if not np.isfinite(wb).all():
                raise ValueError(f"argument 'weights': need {b}: a weight must be finite")
            parts.append(wb)
        if any(wb is not None for wb in wl):
            w = np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)
    V = np.ascontiguousarray(np.concatenate(mats, axis=0), dtype=np.float64)
    return V, offs, w, FUSED_MODES[mode], 1 if on_zero_lambda == "skip" else 0


def _id_lists(lists, nitems: int) -> tuple[np.ndarray, np.ndarray]:
    """B id lists as (ids int64 flat, offsets int64 [B + 1]): a 2-D integer array (B, C) is B lists of C ids; any other
    sequence holds one entry per list, each whatever `_item_ids` accepts (integer ids in any order, duplicates kept, or a
    boolean mask of length nitems).  Non-integer ids raise TypeError."""
    if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.dtype != np.bool_:
        if lists.dtype.kind not in "iu":
            raise TypeError(f"argument 'lists': expected integer item ids or boolean masks, got dtype {lists.dtype}")
        if lists.dtype == np.uint64 and lists.size and int(lists.max()) > np.iinfo(np.int64).max:
            raise ValueError(f"argument 'lists': id {int(lists.max())} is outside [0, {nitems})")
        b, c = lists.shape
        return np.ascontiguousarray(lists, dtype=np.int64).reshape(-1), np.arange(b + 1, dtype=np.int64) * c
    parts = [l if isinstance(l, np.ndarray) and l.ndim == 1 and l.dtype == np.int64 else _item_ids(l, nitems, "lists") for l in lists]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    if parts:
        np.cumsum([p.shape[0] for p in parts], out=offsets[1:])
    ids = np.ascontiguousarray(np.concatenate(parts), dtype=np.int64) if parts else np.empty(0, dtype=np.int64)
    return ids, offsets


class ItemSubset:
    """Extension: a set of items of one ArrowSpace (`ArrowSpace.subset`), resident on the device with every buffer a
    `search_subset` over it needs.  Holds a reference to its ArrowSpace."""

    def __new__(cls, *a, **k):
        raise ValueError("ItemSubset cannot be constructed directly; use ArrowSpace.subset")

    @classmethod
    def _wrap(cls, handle, space):
        self = object.__new__(cls)
        self._h = handle
        self._space = space
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.as_subset_free(h)
            self._h = None
        self._space = None

    @property
    def size(self) -> int:
        """Extension: the number of distinct items in the subset."""
        return int(_L.as_subset_size(self._h))

    def __len__(self) -> int:
        return self.size

    def ids(self) -> np.ndarray:
        """Extension: the subset's item ids, sorted and unique (int64)."""
        out = np.empty(self.size, dtype=np.int64)
        st = _L.as_subset_ids(self._h, out.ctypes.data_as(C.c_void_p))
        _check(st)
        return out

    def set_timing(self, enabled: bool) -> None:
        """Measurement only (tools/subset_bench.py, tools/subset_batch_bench.py, tools/subset_sweep_bench.py): record HIP events around the score kernel of `search_subset` / `search_batch_subset` calls and their `*_taus` sweeps on this subset (off by default)."""
        _L.as_subset_set_timing(self._h, 1 if enabled else 0)

    @property
    def kernel_us(self) -> float:
        """Measurement only: device microseconds of the score kernel in the last timed `search_subset` call on this subset (`search_batch_subset`: summed over the call's chunks; the sweeps: over the call's launches)."""
        return float(_L.as_subset_kernel_us(self._h))


GROUPED_MAX_GROUPS = 1024      # == SUBSET_TOPK of the library
GROUPED_MAX_PER_GROUP = 16     # == GROUPED_MAX_PER_GROUP of the library


def _group_labels(labels, nitems: int) -> np.ndarray:
    """One integer label per item as a contiguous int64 array of nitems entries.  A bool or float dtype (or anything that is
    not an integer) raises TypeError, a wrong rank or length, or a uint64 label past the int64 range, ValueError."""
    a = np.asarray(labels)
    if a.dtype.kind not in "iu":
        raise TypeError(f"argument 'labels': expected one integer label per item, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"argument 'labels': expected a 1-D sequence of {nitems} labels, got shape {a.shape}")
    if a.shape[0] != nitems:
        raise ValueError(f"argument 'labels': {a.shape[0]} labels for {nitems} items")
    if a.dtype == np.uint64 and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"argument 'labels': label {int(a.max())} does not fit int64")
    return np.ascontiguousarray(a, dtype=np.int64)


def _grouped_args(gl, tau, n_groups, per_group):
    """What the grouped forms check before they touch a handle."""
    _need_gl(gl)
    for name, v, hi in (("n_groups", n_groups, GROUPED_MAX_GROUPS), ("per_group", per_group, GROUPED_MAX_PER_GROUP)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"argument '{name}': expected an integer")
        if v < 1 or v > hi:
            raise ValueError(f"argument '{name}': must be in [1, {hi}], got {v}")
    tau = float(tau)
    if not np.isfinite(tau):
        raise ValueError("argument 'tau': must be finite")
    return tau, int(n_groups), int(per_group)


def _group_members(labels):
    """The member table of per-item labels -> (labels int64 [G] ascending and distinct, order int64 [n]: the items by (label
    ascending, item id ascending), starts int64 [G + 1]): the members of the group with labels[g] are order[starts[g]:starts[g + 1]]."""
    lab = np.ascontiguousarray(labels, dtype=np.int64)
    order = np.argsort(lab, kind="stable").astype(np.int64, copy=False)
    uniq, counts = np.unique(lab, return_counts=True)
    starts = np.zeros(uniq.shape[0] + 1, dtype=np.int64)
    np.cumsum(counts, out=starts[1:])
    return uniq, order, starts


def _label_lists(lists, b: int) -> list:
    """The candidate documents of b needs as b contiguous int64 1-D arrays of group labels (the caller's order, duplicates kept):
    a 2-D integer array (B, C) is B lists of C labels, any other sequence holds one 1-D sequence of labels per need (empty ones
    allowed).  TypeError: a float or boolean dtype, something that is no sequence; ValueError: a count of lists other than b, a
    list that is not 1-D, a uint64 label past the int64 range."""
    if isinstance(lists, (str, bytes)) or not hasattr(lists, "__iter__"):
        raise TypeError("argument 'lists': expected one sequence of group labels per need")
    seq = list(lists)
    if len(seq) != b:
        raise ValueError(f"argument 'lists': {len(seq)} label lists for {b} needs")
    parts = []
    for i, l in enumerate(seq):
        if isinstance(l, (str, bytes)):
            raise TypeError(f"argument 'lists': need {i}: expected integer group labels")
        a = np.asarray(l)
        if a.size == 0 and a.ndim == 1 and a.dtype.kind not in "iub":
            a = np.empty(0, dtype=np.int64)
        if a.dtype.kind not in "iu":
            raise TypeError(f"argument 'lists': need {i}: expected integer group labels, got dtype {a.dtype}")
        if a.ndim != 1:
            raise ValueError(f"argument 'lists': need {i}: expected a 1-D sequence of group labels, got shape {a.shape}")
        if a.dtype == np.uint64 and a.size and int(a.max()) > np.iinfo(np.int64).max:
            raise ValueError(f"argument 'lists': label {int(a.max())} is not one of the groups")
        parts.append(np.ascontiguousarray(a, dtype=np.int64))
    return parts


def _expand_documents(parts, members):
    """The documents of every need from its label list (`_label_lists`) and a member table (`_group_members`) -> (need_docs int64
    [B + 1], doc_label int64 [ND], doc_first int64 [ND + 1], ids int64 [NE], inverse: B int64 arrays).  Need b's documents are
    need_docs[b] .. need_docs[b + 1] - 1: the DISTINCT labels of its list, ascending; document dd's entries
    ids[doc_first[dd]:doc_first[dd + 1]] are the members of its group, ascending, so that a need's entries are ordered by (label,
    item id); inverse[b][c] is the document (counted inside need b) of the caller's entry c.  ValueError names a label that is
    not one of the groups."""
    uniq, order, starts = members
    need_docs = np.zeros(len(parts) + 1, dtype=np.int64)
    docs, inverse = [], []
    for b, l in enumerate(parts):
        dl, iv = np.unique(l, return_inverse=True)
        docs.append(dl)
        inverse.append(iv.astype(np.int64, copy=False).reshape(-1))
        need_docs[b + 1] = need_docs[b] + dl.shape[0]
    doc_label = np.ascontiguousarray(np.concatenate(docs), dtype=np.int64) if docs else np.empty(0, dtype=np.int64)
    g = np.searchsorted(uniq, doc_label)
    known = np.zeros(doc_label.shape[0], dtype=bool)
    if uniq.shape[0]:
        known = uniq[np.minimum(g, uniq.shape[0] - 1)] == doc_label
    if not known.all():
        raise ValueError(f"argument 'lists': label {int(doc_label[np.flatnonzero(~known)[0]])} is not one of the groups")
    size = starts[g + 1] - starts[g]
    doc_first = np.zeros(doc_label.shape[0] + 1, dtype=np.int64)
    np.cumsum(size, out=doc_first[1:])
    ne = int(doc_first[-1])
    ids = order[np.repeat(starts[g] - doc_first[:-1], size) + np.arange(ne, dtype=np.int64)]
    return need_docs, doc_label, doc_first, np.ascontiguousarray(ids, dtype=np.int64), inverse


class ItemGroups:
    """Extension: one group per item of one ArrowSpace (`ArrowSpace.groups`): the items' integer labels, turned into dense group
    numbers once and resident on the device for `search_grouped`.  Holds a reference to its ArrowSpace."""

    def __new__(cls, *a, **k):
        raise ValueError("ItemGroups cannot be constructed directly; use ArrowSpace.groups")

    @classmethod
    def _wrap(cls, handle, space, labels):
        self = object.__new__(cls)
        self._h = handle
        self._space = space
        self._labels = labels
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.as_groups_free(h)
            self._h = None
        self._space = None

    @property
    def ngroups(self) -> int:
        """Extension: the number of distinct labels."""
        return int(_L.as_groups_count(self._h))

    def __len__(self) -> int:
        return self.ngroups

    def labels(self) -> np.ndarray:
        """Extension: the per-item labels (int64, a copy)."""
        return self._labels.copy()

    def _members(self):
        """The member table of the labels (`_group_members`), made by the first call that needs it and kept."""
        table = getattr(self, "_member_table", None)
        if table is None:
            table = self._member_table = _group_members(self._labels)
        return table


class ArrowSpace:
    """Items + per-item lambdas resident in HBM (src/lib.rs:64-263)."""

    def __new__(cls, *a, **k):
        raise ValueError("ArrowSpace cannot be constructed directly; use ArrowSpaceBuilder.build")

    @classmethod
    def _wrap(cls, handle):
        self = object.__new__(cls)
        self._h = handle
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.as_free_space(h)
            self._h = None

    @property
    def nitems(self) -> int:
        return int(_L.as_nitems(self._h))

    @property
    def nfeatures(self) -> int:
        return int(_L.as_nfeatures(self._h))

    def get_item(self, idx: int):
        """src/lib.rs:100-120: (features ndarray[float64], lambda)."""
        if isinstance(idx, bool) or not isinstance(idx, (int, np.integer)):
            raise TypeError("idx must be an integer")
        if idx < 0:
            raise OverflowError("can't convert negative int to unsigned")
        out = np.empty(self.nfeatures, dtype=np.float64)
        lam = C.c_double(0.0)
        st = _L.as_get_item(self._h, int(idx), out.ctypes.data_as(C.c_void_p), C.byref(lam))
        if st:
            _raise(st)
        return out, float(lam.value)

    def lambdas(self) -> np.ndarray:
        out = np.empty(self.nitems, dtype=np.float64)
        st = _L.as_lambdas(self._h, out.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        return out

    @staticmethod
    def _query(item) -> np.ndarray:
        # PyReadonlyArray1<f64> + as_slice(): float64, 1-D, contiguous (src/lib.rs:139)
        if not isinstance(item, np.ndarray) or item.dtype != np.float64:
            raise TypeError("argument 'item': expected a 1-D numpy.ndarray of dtype float64")
        if item.ndim != 1:
            raise TypeError("argument 'item': expected a 1-D numpy.ndarray of dtype float64")
        if not item.flags.c_contiguous:
            raise ValueError("The given array is not contiguous")
        return item

    def search(self, item, gl: GraphLaplacian, tau: float):
        """src/lib.rs:132-174: list[(index, score)], length topk, score descending."""
        if not isinstance(gl, GraphLaplacian):
            raise TypeError("argument 'gl': expected GraphLaplacian")
        q = self._query(item)
        # per-(thread, space, graph) call state: output buffers and ctypes arguments are built once.  Per thread,
        # because ctypes drops the GIL during the call: the library serialises searches on a space, but shared
        # output buffers would be overwritten by the next thread's call before this one has read them.
        tls = self.__dict__.get("_tls")
        if tls is None:
            tls = self.__dict__.setdefault("_tls", threading.local())
        st_ = getattr(tls, "s", None)
        if st_ is None or st_[0] is not gl:
            topk = max(min(int(gl.graph_params["topk"]), self.nitems), 1)
            idx = (C.c_int64 * topk)()
            sc = (C.c_double * topk)()
            ln, lq = C.c_int64(0), C.c_double(0.0)
            st_ = tls.s = (gl, idx, sc, ln, lq, C.byref(ln), C.byref(lq))
        _, idx, sc, ln, lq, pln, plq = st_
        st = _L.as_search(self._h, gl._h, q.ctypes.data, q.shape[0], tau, idx, sc, pln, plq)
        if st:
            _raise(st)
        n = ln.value
        return list(zip(idx[:n], sc[:n]))

    def search_batch(self, items, gl: GraphLaplacian, tau: float):
        """Extension: B queries [B, D] -> list of B hit lists."""
        Q = np.ascontiguousarray(items, dtype=np.float64)
        if Q.ndim != 2:
            raise TypeError("items must be a 2-D float64 array")
        topk = min(int(gl.graph_params["topk"]), self.nitems)
        b = Q.shape[0]
        idx = np.empty((b, topk), dtype=np.int64)
        sc = np.empty((b, topk), dtype=np.float64)
        ln = np.zeros(b, dtype=np.int64)
        lq = np.zeros(b, dtype=np.float64)
        stt = np.zeros(b, dtype=np.int32)
        st = _L.as_search_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau),
                                idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                ln.ctypes.data_as(C.c_void_p), lq.ctypes.data_as(C.c_void_p),
                                stt.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        if (stt == _lib.AS_EZEROLAMBDA).any():
            raise PanicException("The lambdas are zero, check the magnitude of items and eps.")
        # (tolist + zip: element-wise int()/float() over the arrays cost 1.5 ms per 256 queries, a fifth of the GPU time)
        return [list(zip(ii, ss)) if l == topk else list(zip(ii[:l], ss[:l]))
                for ii, ss, l in zip(idx.tolist(), sc.tolist(), ln.tolist())]

    def search_taus(self, item, gl: GraphLaplacian, taus):
        """Extension: one query under several taus (a tau sweep) -> one hit list per entry of `taus`, in order; list j is what
        `search(item, gl, taus[j])` returns.  Taus in [0, 1] share passes over the items (up to 8 per pass: one scan, one k-NN
        step, one exact evaluation of the union of the taus' candidates); equal taus are computed once, and a tau outside
        [0, 1], a sweep of one distinct tau, or anything a shared pass does not serve takes the single search."""
        if not isinstance(gl, GraphLaplacian):
            raise TypeError("argument 'gl': expected GraphLaplacian")
        q = self._query(item)
        t = np.ascontiguousarray(taus, dtype=np.float64)
        if t.ndim != 1:
            raise TypeError("argument 'taus': expected a 1-D sequence of floats")
        nt = t.shape[0]
        topk = max(min(int(gl.graph_params["topk"]), self.nitems), 0)
        idx = np.empty((max(nt, 1), max(topk, 1)), dtype=np.int64)
        sc = np.empty((max(nt, 1), max(topk, 1)), dtype=np.float64)
        ln = np.zeros(max(nt, 1), dtype=np.int64)
        lq = C.c_double(0.0)
        st = _L.as_search_taus(self._h, gl._h, q.ctypes.data, q.shape[0], t.ctypes.data, nt, idx.ctypes.data, sc.ctypes.data,
                               ln.ctypes.data, C.byref(lq))
        if st:
            _raise(st)
        idx, sc = idx[:, :topk], sc[:, :topk]
        return [list(zip(ii[:l], ss[:l])) for ii, ss, l in zip(idx[:nt].tolist(), sc[:nt].tolist(), ln[:nt].tolist())]

    def subset(self, ids_or_mask) -> ItemSubset:
        """Extension: an `ItemSubset` of this space from integer item ids (array or sequence, any order, duplicates allowed)
        or a boolean mask of length nitems.  Ids are sorted and made unique once; an id outside [0, nitems) raises
        ValueError, floating-point ids TypeError."""
        ids = _item_ids(ids_or_mask, self.nitems, "ids_or_mask")
        h = C.c_void_p()
        st = _L.as_subset_create(self._h, ids.ctypes.data_as(C.c_void_p), ids.shape[0], C.byref(h))
        _check(st)
        return ItemSubset._wrap(h, self)

    def _as_subset(self, subset, optional=False):
        """An `ItemSubset` as it is, anything `subset()` accepts as a temporary one; optional: None stands for every item."""
        return subset if isinstance(subset, ItemSubset) or (optional and subset is None) else self.subset(subset)

    def _hits_bound(self, gl, sub=None) -> int:
        """Entries of a hit list over the subset (None: every item): min(topk, nitems, |subset|)."""
        return min(int(gl.graph_params["topk"]), self.nitems, self.nitems if sub is None else sub.size)

    def search_subset(self, item, gl: GraphLaplacian, tau: float, subset):
        """Extension: filtered search -> list[(index, score)]: the first min(topk, |subset|) items OF THE SUBSET by (score
        descending, index ascending).  The filter restricts what may be returned, not the index: lambda_q and the items'
        lambdas are the ones `search` uses, and with every item in the subset the result is `search`'s.  `subset`: an
        `ItemSubset` of this space (prepared once, reused over queries) or anything `subset()` accepts (a temporary one is
        made).  Costs one ordinary `search` (lambda_q comes from it; a query whose lambda_q is 0 panics as there, whatever
        the subset) plus a gather of the subset's rows and an exact selection on the device."""
        _need_gl(gl)
        q = self._query(item)
        sub = self._as_subset(subset)
        n = max(min(int(gl.graph_params["topk"]), sub.size), 1)
        idx = np.empty(n, dtype=np.int64)
        sc = np.empty(n, dtype=np.float64)
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = _L.as_search_subset(self._h, gl._h, q.ctypes.data, q.shape[0], float(tau), sub._h, idx.ctypes.data, sc.ctypes.data,
                                 C.byref(ln), C.byref(lq))
        _check(st)
        return list(zip(idx[:ln.value].tolist(), sc[:ln.value].tolist()))

    def score_items(self, item, gl: GraphLaplacian, tau: float, ids) -> np.ndarray:
        """Extension: re-ranking -> ndarray[float64]: entry i is the score `search` would give item ids[i] (the caller's
        order, duplicates kept; integer ids or a boolean mask as for `subset`).  Costs one ordinary `search` (lambda_q) plus
        a gather of the listed rows."""
        _need_gl(gl)
        q = self._query(item)
        ids = _item_ids(ids, self.nitems, "ids")
        out = np.empty(ids.shape[0], dtype=np.float64)
        lq = C.c_double(0.0)
        st = _L.as_score_items(self._h, gl._h, q.ctypes.data, q.shape[0], float(tau), ids.ctypes.data_as(C.c_void_p), ids.shape[0],
                               out.ctypes.data_as(C.c_void_p), C.byref(lq))
        _check(st)
        return out

    def search_batch_subset(self, items, gl: GraphLaplacian, tau: float, subset):
        """Extension: batched filtered search, B queries [B, D] against one subset -> list of B hit lists; list i is what
        `search_subset(items[i], gl, tau, subset)` returns (scores within 1e-12 relative: the batched kernel sums in another
        order; indices equal except inside such ties).  `subset`: an `ItemSubset` of this space or anything `subset()` accepts.
        Costs one `search_batch` over the B queries (lambda_q comes from it; any query whose lambda_q is 0 panics as there,
        whatever the subset), then the subset's rows are gathered once per 64 queries for an fp64 matrix product on the
        device and every query's list is selected there."""
        _need_gl(gl)
        Q = _queries_2d(items)
        sub = self._as_subset(subset)
        b = Q.shape[0]
        kk = self._hits_bound(gl, sub)
        (idx, sc, ln), stt = _hit_buffers(b, kk), _statuses(b)
        st = _L.as_search_subset_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau), sub._h,
                                       idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p),
                                       None, stt.ctypes.data_as(C.c_void_p))
        _check(st, stt, b)
        return _hit_lists(idx, sc, ln, b, kk)

    def score_items_batch(self, items, gl: GraphLaplacian, tau: float, ids) -> np.ndarray:
        """Extension: batched re-ranking -> ndarray[float64] of shape (B, len(ids)): entry [i, j] is what
        `score_items(items[i], gl, tau, ids)[j]` returns (the caller's order, duplicates kept; within 1e-12 relative: the
        batched kernel sums in another order).  Costs one `search_batch` over the B queries (lambda_q; a query whose lambda_q
        is 0 panics as there) plus one gather of the listed rows per 64 queries."""
        _need_gl(gl)
        Q = _queries_2d(items)
        ids = _item_ids(ids, self.nitems, "ids")
        b, m = Q.shape[0], ids.shape[0]
        out = np.empty((b, m), dtype=np.float64)
        stt = _statuses(b)
        st = _L.as_score_items_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau),
                                     ids.ctypes.data_as(C.c_void_p), m, out.ctypes.data_as(C.c_void_p), None,
                                     stt.ctypes.data_as(C.c_void_p))
        _check(st, stt, b)
        return out

    def _range_single(self, item, gl, tau, min_score, subset, count_only):
        _need_gl(gl)
        q = self._query(item)
        if np.ndim(min_score) != 0:
            raise ValueError("argument 'min_score': expected one float")
        thr = float(_min_scores(min_score, 1)[0])
        sub = self._as_subset(subset, optional=True)
        h, lq = C.c_void_p(), C.c_double(0.0)
        st = _L.as_search_range(self._h, gl._h, q.ctypes.data, q.shape[0], float(tau), thr, _handle(sub),
                                1 if count_only else 0, C.byref(h), C.byref(lq))
        _check(st)
        try:
            n = int(_L.as_range_total(h))
            if count_only:
                return n
            idx = np.empty(max(n, 1), dtype=np.int64)
            sc = np.empty(max(n, 1), dtype=np.float64)
            st = _L.as_range_copy(h, idx.ctypes.data, sc.ctypes.data)
            _check(st)
            return list(zip(idx[:n].tolist(), sc[:n].tolist()))
        finally:
            _L.as_range_free(h)

    def _range_batch(self, items, gl, tau, min_score, subset, count_only):
        _need_gl(gl)
        Q = _queries_2d(items)
        b = Q.shape[0]
        thr = _min_scores(min_score, b)
        sub = self._as_subset(subset, optional=True)
        h = C.c_void_p()
        stt = _statuses(b)
        st = _L.as_search_range_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau),
                                      thr.ctypes.data_as(C.c_void_p), _handle(sub), 1 if count_only else 0,
                                      C.byref(h), None, stt.ctypes.data_as(C.c_void_p))
        _check(st)
        try:
            _panic_on_zero_lambda(stt, b)   # (inside the try: the answer's handle is freed)
            offs = np.zeros(b + 1, dtype=np.int64)
            st = _L.as_range_offsets(h, offs.ctypes.data)
            _check(st)
            if count_only:
                return np.diff(offs)
            n = int(offs[b])
            idx = np.empty(max(n, 1), dtype=np.int64)
            sc = np.empty(max(n, 1), dtype=np.float64)
            st = _L.as_range_copy(h, idx.ctypes.data, sc.ctypes.data)
            _check(st)
            idx, sc, o = idx.tolist(), sc.tolist(), offs.tolist()
            return [list(zip(idx[o[i]:o[i + 1]], sc[o[i]:o[i + 1]])) for i in range(b)]
        finally:
            _L.as_range_free(h)

    def search_range(self, item, gl: GraphLaplacian, tau: float, min_score: float, subset=None):
        """Extension: range search -> list[(index, score)]: EVERY item of the subset whose score is >= `min_score`, by (score
        descending, index ascending), not cut at topk; a NaN score never qualifies, `min_score` may be -inf or +inf (NaN
        raises ValueError).  `subset`: None (every item), an `ItemSubset` of this space or anything `subset()` accepts.  The
        filter restricts the answer, not the index, as in `search_subset`; the score of item i has the bits
        `score_items(item, gl, tau, [i])` returns.  Costs one ordinary `search` (lambda_q comes from it; a query whose lambda_q
        is 0 panics as there, whatever the subset and the threshold) plus a gather of the subset's rows and one compaction
        pass over the scores on the device: only the survivors cross to the host, where they are sorted -- an answer of a
        million items is legal and slow."""
        return self._range_single(item, gl, tau, min_score, subset, False)

    def count_range(self, item, gl: GraphLaplacian, tau: float, min_score: float, subset=None) -> int:
        """Extension: the length of `search_range(item, gl, tau, min_score, subset)` without the list.  Costs one ordinary
        `search` (lambda_q) plus a gather of the subset's rows and one counting pass over the scores on the device; one
        number per query crosses to the host."""
        return self._range_single(item, gl, tau, min_score, subset, True)

    def search_range_batch(self, items, gl: GraphLaplacian, tau: float, min_score, subset=None):
        """Extension: batched range search, B queries [B, D] against one subset -> list of B lists; list i is what
        `search_range(items[i], gl, tau, min_score[i], subset)` returns with the score bits of `score_items_batch` (within
        1e-12 relative of the single form's: the batched kernel sums in another order; membership differs only for scores
        that close to the threshold).  `min_score`: one float for every query or a sequence of B floats.  Costs one
        `search_batch` over the B queries (lambda_q comes from it; any query whose lambda_q is 0 panics as there, whatever the
        subset), then the subset's rows are gathered once per 64 queries for an fp64 matrix product on the device and one
        compaction pass per chunk of queries keeps the survivors."""
        return self._range_batch(items, gl, tau, min_score, subset, False)

    def count_range_batch(self, items, gl: GraphLaplacian, tau: float, min_score, subset=None) -> np.ndarray:
        """Extension: ndarray[int64] of B: the lengths of `search_range_batch(items, gl, tau, min_score, subset)`'s lists.
        Costs one `search_batch` over the B queries (lambda_q) plus one gather of the subset's rows per 64 queries and one
        counting pass per chunk of queries."""
        return self._range_batch(items, gl, tau, min_score, subset, True)

    def range_counters(self) -> dict:
        """Extension: range calls on this space since it was made, the work they launched and what they returned."""
        return _counters(_L.as_range_counters, self._h, ("calls", "compactions", "scores_examined", "survivors", "relaunches", "lambda_steps"))

    def search_fused(self, items, gl: GraphLaplacian, tau: float, weights=None, mode="sum", subset=None, on_zero_lambda="raise"):
        """Extension: fused multi-query search, ONE answer to J query vectors [J, D] -> list[(index, score)]: the first
        min(topk, |subset|) items of the subset (None: every item) by (F descending, index ascending).  With s_j(i) the score
        `score_items_batch(items, gl, tau, ids)[j, i]` and t_j(i) = weights[j] * s_j(i) (weights default to 1/J each; negative
        weights are legal), F is, j ascending, mode "sum": t_0, then F + t_j, every product and sum rounded once; mode "max":
        t_0, then t_j where t_j > F or F is NaN -- the numpy loop over `score_items_batch` reproduces the bits.  A vector
        whose lambda_q is 0: on_zero_lambda="raise" panics as `search` does, for the whole call; "skip" leaves that vector out
        (its weight is dropped, the others are not renormalised); no vector left panics in either setting.  J = 1 with weights
        [1.0] returns `search_batch_subset(items, gl, tau, subset)[0]` bit for bit.  Costs one `search_batch` over the J
        vectors (lambda_q), the gather and fp64 matrix product of the batched filtered forms, one pass per chunk of vectors
        that folds the scores into an accumulator on the device, and one exact selection there: topk entries cross to the
        host, the J x M scores never do."""
        Q, w, m, skip = _fused_args(items, gl, weights, mode, on_zero_lambda)
        sub = self._as_subset(subset, optional=True)
        idx, sc, _ = _hit_buffers(1, self._hits_bound(gl, sub))
        ln = C.c_int64(0)
        st = _L.as_search_fused(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), Q.shape[0], Q.shape[1], float(tau),
                                None if w is None else w.ctypes.data_as(C.c_void_p), m, skip, _handle(sub),
                                idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(ln), None, None)
        _check(st)
        return list(zip(idx[:ln.value].tolist(), sc[:ln.value].tolist()))

    def score_fused(self, items, gl: GraphLaplacian, tau: float, ids, weights=None, mode="sum", on_zero_lambda="raise") -> np.ndarray:
        """Extension: the fused score F of `search_fused` (same weights, modes and zero-lambda rule) for each listed id ->
        ndarray[float64] of len(ids): the caller's order, duplicates kept; integer ids or a boolean mask as for `subset`.
        Equals the numpy fold of `score_items_batch(items, gl, tau, ids)` bit for bit.  Costs what `search_fused` costs
        without the selection: the accumulator's len(ids) doubles cross to the host."""
        Q, w, m, skip = _fused_args(items, gl, weights, mode, on_zero_lambda)
        ids = _item_ids(ids, self.nitems, "ids")
        out = np.empty(ids.shape[0], dtype=np.float64)
        st = _L.as_score_fused(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), Q.shape[0], Q.shape[1], float(tau),
                               None if w is None else w.ctypes.data_as(C.c_void_p), m, skip, ids.ctypes.data_as(C.c_void_p), ids.shape[0],
                               out.ctypes.data_as(C.c_void_p), None, None)
        _check(st)
        return out

    def fused_counters(self) -> list:
        """Extension: [0] fused calls on this space that passed their checks, [1] accumulate launches, [2] scores folded
        (served vectors x items), [3] lambda_q steps run."""
        return list(_counters(_L.as_fused_counters, self._h, ("calls", "launches", "folded", "lambda_steps")).values())

    def search_fused_batch(self, needs, gl: GraphLaplacian, tau: float, weights=None, mode="sum", subset=None, on_zero_lambda="raise"):
        """Extension: batched fused search, B needs of J_b query vectors each in ONE call -> list of B lists[(index, score)];
        list b is the fused answer of need b: the first min(topk, |subset|) items by (F descending, index ascending), F the
        fold of `search_fused` over need b's own vectors.  `needs`: a 3-D array (B, J, D), or a sequence of B 2-D arrays
        (J_b, D), the J_b may differ.  `weights`: None (1/J_b each), a (B, J) array, or a sequence of B 1-D sequences of J_b
        finite numbers, a None entry meaning the default for that need.  tau, mode, subset and on_zero_lambda are common to
        the call.  With V the vectors of all needs flattened in need order, the per-vector scores are the bits of
        `score_items_batch(V, gl, tau, ids)` -- lambda_q of every vector comes from ONE `search_batch` over V -- and every
        need's fold is the numpy loop over its rows.  B = 1 is `search_fused` bit for bit; whether a need's answer depends on
        the OTHER needs of the call is `search_batch`'s property and is not promised.  A vector whose lambda_q is 0:
        on_zero_lambda="raise" panics as `search` does, for the whole call, before anything is gathered; "skip" leaves it out
        of its need (the other weights are not renormalised), a need with no vector left gets [] and the other needs are
        served.  Costs one `search_batch` over V, then the subset's rows are gathered once per 64 VECTORS of the call, whatever
        need they belong to, one segmented pass per chunk folds every need's rows into that need's accumulator on the device,
        and one batched selection follows: B x topk entries cross to the host."""
        V, offs, w, m, skip = _fused_batch_args(needs, gl, weights, mode, on_zero_lambda)
        sub = self._as_subset(subset, optional=True)
        b, kk = offs.shape[0] - 1, self._hits_bound(gl, sub)
        (idx, sc, ln), stt = _hit_buffers(b, kk), _statuses(b)
        st = _L.as_search_fused_batch(self._h, gl._h, V.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), b, V.shape[0], V.shape[1],
                                      float(tau), None if w is None else w.ctypes.data_as(C.c_void_p), m, skip, _handle(sub),
                                      idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), None,
                                      stt.ctypes.data_as(C.c_void_p))
        _check(st)
        return _hit_lists(idx, sc, ln, b, kk)

    def score_fused_batch(self, needs, gl: GraphLaplacian, tau: float, ids, weights=None, mode="sum", on_zero_lambda="raise") -> np.ndarray:
        """Extension: the fused scores F of `search_fused_batch` (same needs, weights, modes and zero-lambda rule) for each
        listed id -> ndarray[float64] of shape (B, len(ids)): the caller's order, duplicates kept; integer ids or a boolean
        mask as for `subset`.  Row b equals the numpy fold of need b's rows of `score_items_batch(V, gl, tau, ids)` bit for
        bit; B = 1 is `score_fused`.  Under on_zero_lambda="skip" a need with no vector left gets a row of NaN.  Costs what
        `search_fused_batch` costs without the selection: the B x len(ids) accumulators cross to the host."""
        V, offs, w, m, skip = _fused_batch_args(needs, gl, weights, mode, on_zero_lambda)
        ids = _item_ids(ids, self.nitems, "ids")
        b = offs.shape[0] - 1
        out = np.empty((b, ids.shape[0]), dtype=np.float64)
        st = _L.as_score_fused_batch(self._h, gl._h, V.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), b, V.shape[0], V.shape[1],
                                     float(tau), None if w is None else w.ctypes.data_as(C.c_void_p), m, skip,
                                     ids.ctypes.data_as(C.c_void_p), ids.shape[0], out.ctypes.data_as(C.c_void_p), None, None)
        _check(st)
        return out

    def fused_batch_counters(self) -> dict:
        """Extension: batched fused calls on this space since it was made that passed their checks, their needs, the
        accumulate launches, the scores folded (served vectors x items), the lambda_q steps (one per call) and the need
        groups run."""
        return _counters(_L.as_fused_batch_counters, self._h, ("calls", "needs", "launches", "folded", "lambda_steps", "groups"))

    def groups(self, labels) -> ItemGroups:
        """Extension: an `ItemGroups` of this space from one integer label per item (a 1-D sequence or array of length nitems,
        any int64 values; equal labels mean the same group).  The labels are grouped on the host and uploaded once.  A bool or
        float dtype raises TypeError, a wrong length or rank ValueError."""
        lab = _group_labels(labels, self.nitems)
        h = C.c_void_p()
        st = _L.as_groups_create(self._h, lab.ctypes.data_as(C.c_void_p), lab.shape[0], C.byref(h))
        _check(st)
        return ItemGroups._wrap(h, self, lab.copy())

    def _grouped_handles(self, groups, subset):
        """The groups and the subset of a grouped call as handles of THIS space (ValueError for another space's)."""
        grp = groups if isinstance(groups, ItemGroups) else self.groups(groups)
        if grp._space is not self:
            raise ValueError("argument 'groups': the groups were made for another space")
        sub = self._as_subset(subset, optional=True)
        if sub is not None and sub._space is not self:
            raise ValueError("argument 'subset': the subset was made for another space")
        return grp, sub

    @staticmethod
    def _grouped_lists(ng, pg, ngroups, label, count, idx, sc):
        label, count, idx, sc = label.tolist(), count.tolist(), idx.reshape(-1, pg).tolist(), sc.reshape(-1, pg).tolist()
        return [(label[s], list(zip(idx[s][:count[s]], sc[s][:count[s]]))) for s in range(ngroups)]

    def search_grouped(self, item, gl: GraphLaplacian, tau: float, groups, n_groups: int, per_group: int = 1, subset=None):
        """Extension: grouped search -> list[(label, list[(index, score)])]: the best items of the best groups.  Items are
        ordered by (score descending, index ascending), an item whose score is NaN belongs to no answer; a group's members
        are its items inside the subset in that order, groups are ordered by their first member.  Returned: the first
        min(n_groups, groups with a member) groups, each with its label and its first min(per_group, members) members;
        1 <= n_groups <= 1024, 1 <= per_group <= 16.  `groups`: an `ItemGroups` of this space or anything `groups()` accepts;
        `subset`: None (every item), an `ItemSubset` of this space or anything `subset()` accepts -- it restricts the answer,
        not the index, as in `search_subset`.  The score of item i has the bits `score_items(item, gl, tau, [i])` returns.
        Costs one ordinary `search` (lambda_q comes from it; a query whose lambda_q is 0 panics as there, whatever the labels
        and the subset) plus a gather of the subset's rows, two passes over the scores per member rank that pick every
        group's next member with atomics on the device, and one exact selection of the groups there: n_groups x per_group
        entries cross to the host, the scores never do."""
        tau, ng, pg = _grouped_args(gl, tau, n_groups, per_group)
        q = self._query(item)
        grp, sub = self._grouped_handles(groups, subset)
        label, count = np.zeros(ng, dtype=np.int64), np.zeros(ng, dtype=np.int64)
        idx, sc = np.zeros(ng * pg, dtype=np.int64), np.zeros(ng * pg, dtype=np.float64)
        n, lq = C.c_int64(0), C.c_double(0.0)
        st = _L.as_search_grouped(self._h, gl._h, q.ctypes.data, q.shape[0], tau, grp._h, ng, pg, _handle(sub),
                                  label.ctypes.data, count.ctypes.data, idx.ctypes.data, sc.ctypes.data, C.byref(n), C.byref(lq))
        _check(st)
        return self._grouped_lists(ng, pg, n.value, label, count, idx, sc)

    def search_batch_grouped(self, items, gl: GraphLaplacian, tau: float, groups, n_groups: int, per_group: int = 1, subset=None):
        """Extension: batched grouped search, B queries [B, D] -> list of B answers; answer i is what
        `search_grouped(items[i], gl, tau, groups, n_groups, per_group, subset)` returns with the score bits of
        `score_items_batch` (within 1e-12 relative of the single form's: the batched kernel sums in another order).  B = 0
        returns [] and launches nothing.  Costs one `search_batch` over the B queries (lambda_q comes from it; any query whose
        lambda_q is 0 panics as there), then per chunk of queries the batched filtered forms' gather and fp64 matrix product
        and the pick passes, the selection and the gather of `search_grouped` with one row per query."""
        tau, ng, pg = _grouped_args(gl, tau, n_groups, per_group)
        Q = _queries_2d(items)
        b = Q.shape[0]
        if b == 0:
            return []
        grp, sub = self._grouped_handles(groups, subset)
        label, count = np.zeros((b, ng), dtype=np.int64), np.zeros((b, ng), dtype=np.int64)
        idx, sc = np.zeros((b, ng * pg), dtype=np.int64), np.zeros((b, ng * pg), dtype=np.float64)
        n, stt = np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int32)
        st = _L.as_search_grouped_batch(self._h, gl._h, Q.ctypes.data, b, Q.shape[1], tau, grp._h, ng, pg, _handle(sub),
                                        label.ctypes.data, count.ctypes.data, idx.ctypes.data, sc.ctypes.data, n.ctypes.data, None,
                                        stt.ctypes.data)
        _check(st, stt, b)
        return [self._grouped_lists(ng, pg, int(n[i]), label[i], count[i], idx[i], sc[i]) for i in range(b)]

    def grouped_counters(self) -> dict:
        """Extension: grouped calls on this space since it was made, the work they launched and what they returned."""
        return _counters(_L.as_grouped_counters, self._h,
                         ("calls", "pick_launches", "scores_examined", "max_atomics", "groups", "members", "lambda_steps"))

    def _maxsim_args(self, items, gl, tau, groups, n_groups, weights, subset, on_zero_lambda):
        """What the late-interaction forms check before they touch a handle: the fused forms' checks (vectors, weights, the
        zero-lambda setting), then the grouped forms' (n_groups, tau, handles of this space)."""
        Q, w, _, skip = _fused_args(items, gl, weights, "sum", on_zero_lambda)
        tau, ng, _ = _grouped_args(gl, tau, n_groups, 1)
        grp, sub = self._grouped_handles(groups, subset)
        return Q, w, skip, tau, ng, grp, sub

    @staticmethod
    def _maxsim_labels(labels, grp) -> np.ndarray:
        """The listed group labels of a score form as int64 [L] contiguous.  TypeError: a float or boolean dtype; ValueError: a
        wrong rank, a label that is not one of the groups."""
        lab = np.asarray(labels)
        if lab.size == 0 and lab.ndim == 1:
            lab = np.empty(0, dtype=np.int64)
        if lab.dtype.kind not in "iu":
            raise TypeError(f"argument 'labels': expected integer group labels, got dtype {lab.dtype}")
        if lab.ndim != 1:
            raise ValueError(f"argument 'labels': expected a 1-D sequence of group labels, got shape {lab.shape}")
        known = np.isin(lab, grp._labels)
        if not known.all():
            raise ValueError(f"argument 'labels': label {int(lab[np.flatnonzero(~known)[0]])} is not one of the groups")
        return np.ascontiguousarray(lab, dtype=np.int64)

    def search_maxsim(self, items, gl: GraphLaplacian, tau: float, groups, n_groups: int, weights=None, subset=None, on_zero_lambda="raise"):
        """Extension: late-interaction search (MaxSim), ONE answer to J query vectors [J, D] over GROUPS of items ->
        list[(label, F)]: the first min(n_groups, groups with a non-NaN F) groups by (F descending, label ascending),
        1 <= n_groups <= 1024.  With s_j(i) the score `score_items_batch(items, gl, tau, ids)[j, i]`, m_j(g) is the largest
        s_j over the members of g -- its items inside the subset (None: every item) whose s_j is not NaN; +0.0 where the
        largest is a zero; NaN where g has no member -- and F(g) is `search_fused`'s "sum" fold of weights[j] * m_j(g): j
        ascending, the first served term, then F + t_j, every product and sum rounded once (weights default to 1/J each;
        negative weights are legal).  The numpy group-by over `score_items_batch` reproduces the bits.  `groups`: an
        `ItemGroups` of this space or anything `groups()` accepts; `subset`: as in `search_grouped`.  A vector whose lambda_q
        is 0: `search_fused`'s rule (on_zero_lambda="raise" panics for the whole call before anything is gathered, "skip"
        leaves the vector out with its weight, no vector left panics).  J = 1 with weights [1.0] names the heads of
        `search_batch_grouped`; every item its own group is `search_fused`.  Costs one `search_batch` over the J vectors
        (lambda_q), the gather and fp64 matrix product of the batched filtered forms, per chunk of vectors one pass that
        takes every group's maximum with atomics on the device and one pass that folds the J x G maxima into an accumulator
        there, and one exact selection: n_groups entries cross to the host, the J x M scores never do."""
        Q, w, skip, tau, ng, grp, sub = self._maxsim_args(items, gl, tau, groups, n_groups, weights, subset, on_zero_lambda)
        label, sc = np.zeros(ng, dtype=np.int64), np.zeros(ng, dtype=np.float64)
        ln = C.c_int64(0)
        st = _L.as_search_maxsim(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), Q.shape[0], Q.shape[1], tau,
                                 None if w is None else w.ctypes.data_as(C.c_void_p), skip, grp._h, ng, _handle(sub),
                                 label.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(ln), None, None)
        _check(st)
        return list(zip(label[:ln.value].tolist(), sc[:ln.value].tolist()))

    def score_maxsim(self, items, gl: GraphLaplacian, tau: float, groups, labels, weights=None, subset=None, on_zero_lambda="raise") -> np.ndarray:
        """Extension: the late-interaction score F of `search_maxsim` (same weights, subset and zero-lambda rule) for each
        listed group label -> ndarray[float64] of len(labels): the caller's order, duplicates kept, NaN for a group without a
        member inside the subset.  A label that is not one of the groups raises ValueError.  Costs what `search_maxsim`
        costs without the selection: the accumulator's G doubles cross to the host."""
        Q, w, skip, tau, _, grp, sub = self._maxsim_args(items, gl, tau, groups, 1, weights, subset, on_zero_lambda)
        lab = self._maxsim_labels(labels, grp)
        out = np.empty(lab.shape[0], dtype=np.float64)
        st = _L.as_score_maxsim(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), Q.shape[0], Q.shape[1], tau,
                                None if w is None else w.ctypes.data_as(C.c_void_p), skip, grp._h, _handle(sub),
                                lab.ctypes.data_as(C.c_void_p), lab.shape[0], out.ctypes.data_as(C.c_void_p), None, None)
        _check(st)
        return out

    def maxsim_counters(self) -> dict:
        """Extension: late-interaction calls on this space since it was made that passed their checks, the vectors they
        served, the group-maximum (pass A) launches, the 64-bit max-atomics those issued and the fold launches."""
        return _counters(_L.as_maxsim_counters, self._h, ("calls", "vectors_served", "pass_a_launches", "max_atomics", "fold_launches"))

    def _maxsim_batch_args(self, needs, gl, tau, groups, n_groups, weights, subset, on_zero_lambda):
        """What the batched late-interaction forms check before they touch a handle: the batched fused forms' checks (needs,
        weights, the zero-lambda setting), then the grouped forms' (n_groups, tau, handles of this space)."""
        V, offs, w, _, skip = _fused_batch_args(needs, gl, weights, "sum", on_zero_lambda)
        tau, ng, _ = _grouped_args(gl, tau, n_groups, 1)
        grp, sub = self._grouped_handles(groups, subset)
        return V, offs, w, skip, tau, ng, grp, sub

    def search_maxsim_batch(self, needs, gl: GraphLaplacian, tau: float, groups, n_groups: int, weights=None, subset=None,
                            on_zero_lambda="raise"):
        """Extension: batched late-interaction search, B needs of J_b query vectors each in ONE call -> list of B
        lists[(label, F)]; list b is `search_maxsim`'s answer for need b: the first min(n_groups, groups with a non-NaN F_b)
        groups by (F_b descending, label ascending), 1 <= n_groups <= 1024.  `needs` and `weights` are `search_fused_batch`'s:
        a 3-D array (B, J, D) or a sequence of B 2-D arrays (J_b, D), the J_b may differ; weights None (1/J_b each), a (B, J)
        array, or a sequence of B 1-D sequences of J_b finite numbers, a None entry meaning the default for that need.
        `groups` and `subset` are `search_maxsim`'s; they, tau, n_groups and on_zero_lambda are common to the call.  With V
        the vectors of all needs flattened in need order, the per-vector scores are the bits of `score_items_batch(V, gl,
        tau, ids)` -- lambda_q of every vector comes from ONE `search_batch` over V -- the group maxima are `search_maxsim`'s
        per flattened vector, and F_b is the fold over need b's OWN served rows, ascending.  B = 1 is `search_maxsim` bit for
        bit; with every J_b = 1 and weight 1.0 the call names the heads of `search_batch_grouped`; with every item its own
        group it is `search_fused_batch` in "sum" mode; whether a need's answer depends on the OTHER needs of the call is
        `search_batch`'s property and is not promised.  A vector whose lambda_q is 0: on_zero_lambda="raise" panics as
        `search` does, for the whole call, before anything is gathered; "skip" leaves it out of its need (the other weights
        are not renormalised), a need with no vector left gets [] and the other needs are served.  Costs one `search_batch`
        over V, then the subset's rows are gathered once per 64 VECTORS of the call, whatever need they belong to; per chunk
        one group-maximum pass per run of served vectors and ONE segmented pass that folds every need's maxima into that
        need's accumulator on the device; one batched selection follows: B x n_groups entries cross to the host."""
        V, offs, w, skip, tau, ng, grp, sub = self._maxsim_batch_args(needs, gl, tau, groups, n_groups, weights, subset, on_zero_lambda)
        b = offs.shape[0] - 1
        (label, sc, ln), stt = _hit_buffers(b, ng), _statuses(b)
        st = _L.as_search_maxsim_batch(self._h, gl._h, V.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), b, V.shape[0], V.shape[1],
                                       tau, None if w is None else w.ctypes.data_as(C.c_void_p), skip, grp._h, ng, _handle(sub),
                                       label.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), None,
                                       stt.ctypes.data_as(C.c_void_p))
        _check(st)
        return _hit_lists(label, sc, ln, b, ng)

    def score_maxsim_batch(self, needs, gl: GraphLaplacian, tau: float, groups, labels, weights=None, subset=None,
                           on_zero_lambda="raise") -> np.ndarray:
        """Extension: the late-interaction scores F_b of `search_maxsim_batch` (same needs, weights, subset and zero-lambda
        rule) for each listed group label -> ndarray[float64] of shape (B, len(labels)): the caller's order, duplicates kept,
        NaN for a group without a member inside the subset.  A label that is not one of the groups raises ValueError.  B = 1
        is `score_maxsim`.  Under on_zero_lambda="skip" a need with no vector left gets a row of NaN.  Costs what
        `search_maxsim_batch` costs without the selection: the listed groups are picked on the device and B x len(labels)
        doubles cross to the host, the B x G accumulators never do."""
        V, offs, w, skip, tau, _, grp, sub = self._maxsim_batch_args(needs, gl, tau, groups, 1, weights, subset, on_zero_lambda)
        lab = self._maxsim_labels(labels, grp)
        b = offs.shape[0] - 1
        out = np.empty((b, lab.shape[0]), dtype=np.float64)
        st = _L.as_score_maxsim_batch(self._h, gl._h, V.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), b, V.shape[0], V.shape[1],
                                      tau, None if w is None else w.ctypes.data_as(C.c_void_p), skip, grp._h, _handle(sub),
                                      lab.ctypes.data_as(C.c_void_p), lab.shape[0], out.ctypes.data_as(C.c_void_p), None, None)
        _check(st)
        return out

    def maxsim_batch_counters(self) -> dict:
        """Extension: batched late-interaction calls on this space since it was made that passed their checks, their needs,
        the vectors they served, the group-maximum (pass A) launches, the 64-bit max-atomics those issued, the fold launches,
        the lambda_q steps (one per call) and the need groups run."""
        return _counters(_L.as_maxsim_batch_counters, self._h,
                         ("calls", "needs", "vectors_served", "pass_a_launches", "max_atomics", "fold_launches", "lambda_steps", "need_groups"))

    def _maxsim_lists_args(self, needs, gl, tau, groups, n_groups, lists, weights, on_zero_lambda):
        """What the per-need document forms check before they touch a handle: the batched fused forms' checks (needs, weights,
        the zero-lambda setting), the grouped forms' (n_groups, tau), the label lists (`_label_lists`); then the groups as a
        handle of this space and the documents expanded into their members (`_expand_documents`: ValueError for an unknown
        label)."""
        V, offs, w, _, skip = _fused_batch_args(needs, gl, weights, "sum", on_zero_lambda)
        tau, ng, _ = _grouped_args(gl, tau, n_groups, 1)
        parts = _label_lists(lists, offs.shape[0] - 1)
        grp, _ = self._grouped_handles(groups, None)
        return V, offs, w, skip, tau, ng, grp, _expand_documents(parts, grp._members())

    def search_maxsim_lists(self, needs, gl: GraphLaplacian, tau: float, groups, n_groups: int, lists, weights=None, on_zero_lambda="raise"):
        """Extension: late-interaction re-ranking of per-need candidate documents, B needs of J_b query vectors EACH WITH ITS OWN
        list of candidate groups -> list of B lists[(label, F)]; list b holds the first min(n_groups, documents of need b with
        a non-NaN F_b) of need b's distinct candidates by (F_b descending, label ascending), 1 <= n_groups <= 1024.  `needs`,
        `weights` and `on_zero_lambda` are `search_maxsim_batch`'s, `groups` an `ItemGroups` of this space or anything
        `groups()` accepts.  `lists`: B sequences of group LABELS (any order, duplicates and empty lists allowed, needs may share
        labels) or an integer (B, C) array; a float or boolean dtype raises TypeError, a label that is not one of the groups
        or a count of lists other than B ValueError.  There is no subset: the candidates are the filter.  With V the vectors
        of all needs flattened in need order and ids_b the members of need b's candidates by (label, item id), the score of a
        vector v of need b and an item of ids_b has the bits `score_lists_batch(V, gl, tau, [ids_need(v) for v in V])` writes
        (the single forms' summation order; lambda_q of every vector from ONE `search_batch` over V); maxima, fold and the
        zero-lambda rule are `search_maxsim_batch`'s, the fold over need b's own served vectors.  An answer does not depend on
        the order of or duplicates in `lists[b]`, on the other needs' lists, on the chunk budget or the grid.  Against
        `score_maxsim_batch` over the same members as a subset F agrees to 1e-12 relative (non-negative weights), not in bits.
        Costs one `search_batch` over V, then per chunk of needs ONE ragged launch that gathers every candidate row once per
        tile of the need's vectors (`maxsim_lists_geometry`), one launch that takes the per-document maxima and folds them, and
        one selection, all on the device: B x n_groups entries cross to the host, the scores never do."""
        V, offs, w, skip, tau, ng, grp, docs = self._maxsim_lists_args(needs, gl, tau, groups, n_groups, lists, weights, on_zero_lambda)
        need_docs, doc_label, doc_first, ids, _ = docs
        b = offs.shape[0] - 1
        (label, sc, ln), stt = _hit_buffers(b, ng), _statuses(b)
        vp = C.c_void_p
        st = _L.as_search_maxsim_lists(self._h, gl._h, V.ctypes.data_as(vp), offs.ctypes.data_as(vp), b, V.shape[0], V.shape[1], tau,
                                       None if w is None else w.ctypes.data_as(vp), skip, grp._h, ng, need_docs.ctypes.data_as(vp),
                                       doc_label.ctypes.data_as(vp), doc_first.ctypes.data_as(vp), ids.ctypes.data_as(vp),
                                       label.ctypes.data_as(vp), sc.ctypes.data_as(vp), ln.ctypes.data_as(vp), None, stt.ctypes.data_as(vp))
        _check(st)
        return _hit_lists(label, sc, ln, b, ng)

    def score_maxsim_lists(self, needs, gl: GraphLaplacian, tau: float, groups, lists, weights=None, on_zero_lambda="raise"):
        """Extension: the scores F_b of `search_maxsim_lists` (same needs, weights and zero-lambda rule) for every entry of
        `lists[b]` -> a list of B float64 arrays in the caller's order, duplicates kept (an integer (B, C) array as `lists`
        returns an array (B, C)); NaN for a document whose members all score NaN and, under on_zero_lambda="skip", for every
        entry of a need with no vector left; an empty list gives an empty array.  Costs what `search_maxsim_lists` costs
        without the selection: one double per (need, distinct document) crosses to the host."""
        V, offs, w, skip, tau, _, grp, docs = self._maxsim_lists_args(needs, gl, tau, groups, 1, lists, weights, on_zero_lambda)
        need_docs, doc_label, doc_first, ids, inverse = docs
        b = offs.shape[0] - 1
        F = np.empty(max(doc_label.shape[0], 1), dtype=np.float64)
        vp = C.c_void_p
        st = _L.as_score_maxsim_lists(self._h, gl._h, V.ctypes.data_as(vp), offs.ctypes.data_as(vp), b, V.shape[0], V.shape[1], tau,
                                      None if w is None else w.ctypes.data_as(vp), skip, grp._h, need_docs.ctypes.data_as(vp),
                                      doc_label.ctypes.data_as(vp), doc_first.ctypes.data_as(vp), ids.ctypes.data_as(vp),
                                      F.ctypes.data_as(vp), None, None)
        _check(st)
        out = [F[need_docs[i]:need_docs[i + 1]][inverse[i]] for i in range(b)]
        if isinstance(lists, np.ndarray) and lists.ndim == 2:
            return np.stack(out).reshape(lists.shape)
        return out

    def maxsim_lists_counters(self) -> dict:
        """Extension: `search_maxsim_lists` / `score_maxsim_lists` calls on this space that passed their checks, their needs,
        the vectors they served, the score-kernel launches, the rows those were asked to gather (per need: entries x vector
        tiles), the (vector, row) dots, the fold launches, the lambda_q steps (one per call) and the host nanoseconds spent on
        the document checks and the work tables."""
        return _counters(_L.as_maxsim_lists_counters, self._h,
                         ("calls", "needs", "vectors_served", "score_launches", "row_reads", "pairs", "fold_launches", "lambda_steps", "host_ns"))

    def maxsim_lists_geometry(self) -> dict:
        """Extension: the score kernel's geometry of `search_maxsim_lists` on this space: `tile`, the vectors of a need staged
        together (every candidate row is gathered once per tile), and `segment`, the entries of a work item at most."""
        t, r = C.c_int64(0), C.c_int64(0)
        _check(_L.as_maxsim_lists_geometry(self._h, C.byref(t), C.byref(r)))
        return {"tile": int(t.value), "segment": int(r.value)}

    @staticmethod
    def _diverse_params(n, diversity) -> tuple[int, float]:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise TypeError("argument 'n': expected an integer")
        if n < 1:
            raise ValueError(f"n must be >= 1, got {n}")
        delta = float(diversity)
        if not 0.0 <= delta <= 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"diversity must lie in [0, 1], got {diversity}")
        return int(n), delta

    def search_diverse(self, item, gl: GraphLaplacian, tau: float, n: int, diversity: float, subset=None, with_margins=False):
        """Extension: diversified search (greedy maximal marginal relevance) -> list[(index, score)], or list[(index, score,
        margin)] with `with_margins`: min(n, P) items of the POOL, the hit list of `search` (of `search_subset` with a subset;
        P <= topk: build with topk = the pool you want, <= 1024).  Each step picks the unselected pool entry with the largest
        margin (1 - diversity) * score - diversity * (largest cosine with an item picked so far; 0 for the first pick), ties to
        the earlier pool entry; cosines are not clamped.  diversity = 0 returns the first entries of the pool as they are; the
        first pick is always the pool's best hit; scores are the pool's, bit for bit.  n < 1 and a diversity outside [0, 1]
        raise ValueError.  Costs one ordinary `search` / `search_subset` (a query whose lambda_q is 0 panics as there) plus
        one upload of the pool, one launch that runs the whole greedy on the device and one download."""
        _need_gl(gl)
        q = self._query(item)
        n, delta = self._diverse_params(n, diversity)
        sub = self._as_subset(subset, optional=True)
        nn = max(min(n, self._hits_bound(gl, sub)), 1)
        idx = np.empty(nn, dtype=np.int64)
        sc = np.empty(nn, dtype=np.float64)
        mg = np.empty(nn, dtype=np.float64)
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = _L.as_search_diverse(self._h, gl._h, q.ctypes.data, q.shape[0], float(tau), n, delta, _handle(sub),
                                  idx.ctypes.data, sc.ctypes.data, mg.ctypes.data, C.byref(ln), C.byref(lq))
        _check(st)
        k = ln.value
        if with_margins:
            return list(zip(idx[:k].tolist(), sc[:k].tolist(), mg[:k].tolist()))
        return list(zip(idx[:k].tolist(), sc[:k].tolist()))

    def search_batch_diverse(self, items, gl: GraphLaplacian, tau: float, n: int, diversity: float, subset=None, with_margins=False):
        """Extension: batched diversified search, B queries [B, D] -> list of B lists; list i is what `search_diverse` returns
        over the pool `search_batch` (with a subset: `search_batch_subset`) gives query i.  A query whose lambda_q is 0 gets
        an empty list, the others are served.  Costs one `search_batch` / `search_batch_subset` over the B queries, then per
        4096 queries one upload of the pools, one launch (a block per query runs its whole greedy) and one download."""
        _need_gl(gl)
        Q = _queries_2d(items)
        n, delta = self._diverse_params(n, diversity)
        sub = self._as_subset(subset, optional=True)
        b = Q.shape[0]
        nn = min(n, self._hits_bound(gl, sub))
        (idx, sc, ln), stt = _hit_buffers(b, nn), _statuses(b)
        mg = np.empty_like(sc)
        st = _L.as_search_diverse_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau), n, delta,
                                        _handle(sub), idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                        mg.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), None, stt.ctypes.data_as(C.c_void_p))
        _check(st)
        if nn == 0:
            return [[] for _ in range(b)]
        # (the C ABI's lists are at stride nn)
        idx, sc, mg = (a.reshape(-1)[:b * nn].reshape(b, nn).tolist() for a in (idx, sc, mg))
        if with_margins:
            return [list(zip(ii[:l], ss[:l], mm[:l])) for ii, ss, mm, l in zip(idx, sc, mg, ln[:b].tolist())]
        return [list(zip(ii[:l], ss[:l])) for ii, ss, l in zip(idx, sc, ln[:b].tolist())]

    def diverse_counters(self) -> dict:
        """Extension: diversified calls on this space since it was made and the work they launched."""
        return _counters(_L.as_diverse_counters, self._h, ("calls", "launches", "picks", "dots", "pool_steps"))

    @staticmethod
    def _diffuse_params(alpha, steps) -> tuple[float, int]:
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
            raise ValueError(f"steps must be an integer in [0, 64], got {steps!r}")
        if not 0 <= steps <= 64:
            raise ValueError(f"steps must lie in [0, 64], got {steps}")
        a = float(alpha)
        if not 0.0 <= a < 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"alpha must lie in [0, 1), got {alpha}")
        return a, int(steps)

    @staticmethod
    def _diffuse_seeds(seeds, nitems: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """B pairs (ids, values) as (ids int64 flat, values float64 flat, offsets int64 [B + 1]); every check of `diffuse`."""
        ids_parts, val_parts = [], []
        for i, pair in enumerate(seeds):
            try:
                ids, vals = pair
            except (TypeError, ValueError):
                raise ValueError(f"argument 'seeds': entry {i}: expected a pair (ids, values)") from None
            ids = np.asarray(ids)
            if ids.size == 0:
                ids = ids.astype(np.int64)
            if ids.dtype.kind not in "iu":
                raise TypeError(f"argument 'seeds': entry {i}: expected integer item ids, got dtype {ids.dtype}")
            vals = np.ascontiguousarray(vals, dtype=np.float64)
            if ids.ndim != 1 or vals.ndim != 1 or ids.shape[0] != vals.shape[0]:
                raise ValueError(f"argument 'seeds': entry {i}: expected as many values as ids, got shapes {ids.shape} and {vals.shape}")
            if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= nitems):
                raise ValueError(f"argument 'seeds': entry {i}: an id is outside [0, {nitems})")
            if np.unique(ids).shape[0] != ids.shape[0]:
                raise ValueError(f"argument 'seeds': entry {i}: the ids must be distinct")
            if not np.isfinite(vals).all():
                raise ValueError(f"argument 'seeds': entry {i}: a value is not finite")
            ids_parts.append(ids.astype(np.int64))
            val_parts.append(vals)
        offs = np.zeros(len(ids_parts) + 1, dtype=np.int64)
        if ids_parts:
            np.cumsum([p.shape[0] for p in ids_parts], out=offs[1:])
        ids = np.ascontiguousarray(np.concatenate(ids_parts), dtype=np.int64) if ids_parts else np.empty(0, dtype=np.int64)
        vals = np.ascontiguousarray(np.concatenate(val_parts), dtype=np.float64) if val_parts else np.empty(0, dtype=np.float64)
        return ids, vals, offs

    def search_diffuse(self, item, gl: GraphLaplacian, tau: float, alpha: float, steps: int, subset=None):
        """Extension: graph-diffusion search (manifold ranking over the index's k-NN graph) -> list[(index, f)]: the first
        min(topk, |subset|) items of the subset (None: every item) by (f descending, index ascending).  The hit list of
        `search` (of `search_subset` with a subset) seeds y (y[index] = score, a non-finite score left out), and
        f <- alpha * S f + (1 - alpha) * y runs `steps` times from f = y over the WHOLE item graph, S = D^-1/2 A D^-1/2 (the
        off-diagonal of `gl.to_csr()`, sign flipped), every row summed in CSR order, every product and sum rounded once, so f
        has the bits of the numpy recurrence.  Items near the best hits on the graph rise even when their own score is
        modest.  steps = 0 or alpha = 0 gives f = y.  The subset restricts the seeds and the answer, not the diffusion.
        0 <= alpha < 1, 0 <= steps <= 64 (an integer), else ValueError; a feature-mode or row-sharded index raises
        ValueError.  Costs one ordinary `search` / `search_subset` (a query whose lambda_q is 0 panics as there), then
        `steps` passes over the graph's CSR on the device and one exact selection there: only the list crosses."""
        _need_gl(gl)
        q = self._query(item)
        a, steps = self._diffuse_params(alpha, steps)
        sub = self._as_subset(subset, optional=True)
        n = max(self._hits_bound(gl, sub), 1)
        idx = np.empty(n, dtype=np.int64)
        sc = np.empty(n, dtype=np.float64)
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = _L.as_search_diffuse(self._h, gl._h, q.ctypes.data, q.shape[0], float(tau), a, steps, _handle(sub), idx.ctypes.data,
                                  sc.ctypes.data, C.byref(ln), C.byref(lq))
        _check(st)
        return list(zip(idx[:ln.value].tolist(), sc[:ln.value].tolist()))

    def search_batch_diffuse(self, items, gl: GraphLaplacian, tau: float, alpha: float, steps: int, subset=None):
        """Extension: batched graph-diffusion search, B queries [B, D] -> list of B lists; list i is `search_diffuse` over the
        pool `search_batch` (with a subset: `search_batch_subset`) gives query i.  A query's f depends on its own seeds,
        alpha, steps and the graph only.  A query whose lambda_q is 0 gets an empty list, the others are served.  Costs one
        `search_batch` / `search_batch_subset`, then per chunk of 16 or 64 queries `steps` passes over the CSR that serve the
        whole chunk, and one selection."""
        _need_gl(gl)
        Q = _queries_2d(items)
        a, steps = self._diffuse_params(alpha, steps)
        sub = self._as_subset(subset, optional=True)
        b = Q.shape[0]
        kk = self._hits_bound(gl, sub)
        (idx, sc, ln), stt = _hit_buffers(b, kk), _statuses(b)
        vp = C.c_void_p
        st = _L.as_search_diffuse_batch(self._h, gl._h, Q.ctypes.data_as(vp), b, Q.shape[1], float(tau), a, steps, _handle(sub),
                                        idx.ctypes.data_as(vp), sc.ctypes.data_as(vp), ln.ctypes.data_as(vp), None, stt.ctypes.data_as(vp))
        _check(st)
        return _hit_lists(idx, sc, ln, b, kk)

    def score_diffuse(self, item, gl: GraphLaplacian, tau: float, alpha: float, steps: int, ids) -> np.ndarray:
        """Extension: f of `search_diffuse` (no subset) at the listed ids -> ndarray[float64] of shape (len(ids),), the caller's
        order, duplicates kept.  A query whose lambda_q is 0 panics as `search` does.  Only len(ids) doubles cross."""
        q = self._query(item)
        out = self._score_diffuse(q.reshape(1, -1), gl, tau, alpha, steps, ids, True)
        return out[0]

    def score_diffuse_batch(self, items, gl: GraphLaplacian, tau: float, alpha: float, steps: int, ids) -> np.ndarray:
        """Extension: f of `search_batch_diffuse` (no subset) at the listed ids -> ndarray[float64] of shape (B, len(ids)); a
        query whose lambda_q is 0 gets a row of NaN, the others are served."""
        return self._score_diffuse(_queries_2d(items), gl, tau, alpha, steps, ids, False)

    def _score_diffuse(self, Q, gl, tau, alpha, steps, ids, panic):
        _need_gl(gl)
        a, steps = self._diffuse_params(alpha, steps)
        ids = _item_ids(ids, self.nitems, "ids")
        b, m = Q.shape[0], ids.shape[0]
        out = np.empty((b, m), dtype=np.float64)
        stt = _statuses(b)
        vp = C.c_void_p
        st = _L.as_score_diffuse_batch(self._h, gl._h, Q.ctypes.data_as(vp), b, Q.shape[1], float(tau), a, steps, ids.ctypes.data_as(vp), m,
                                       out.ctypes.data_as(vp), None, stt.ctypes.data_as(vp))
        _check(st, stt if panic else None, b)
        return out

    def diffuse(self, gl: GraphLaplacian, seeds, alpha: float, steps: int) -> np.ndarray:
        """Extension: the raw form of graph diffusion -> ndarray[float64] of shape (B, nitems): row b is f after `steps` steps
        of the recurrence of `search_diffuse` from the seeds of `seeds[b]`, a pair (ids, values): y[ids[j]] = values[j], 0
        elsewhere.  The ids of a pair must be distinct and inside [0, nitems) and the values finite (ValueError); a float or
        boolean dtype of ids raises TypeError.  It runs the recurrence and nothing else: no search, no selection.  The whole
        B x nitems block crosses to the host (8 MB per query at a million items): use `score_diffuse` or `search_diffuse`
        where a few entries are wanted."""
        _need_gl(gl)
        a, steps = self._diffuse_params(alpha, steps)
        ids, vals, offs = self._diffuse_seeds(seeds, self.nitems)
        b = offs.shape[0] - 1
        out = np.empty((b, self.nitems), dtype=np.float64)
        vp = C.c_void_p
        st = _L.as_diffuse_seeds(self._h, gl._h, ids.ctypes.data_as(vp), vals.ctypes.data_as(vp), offs.ctypes.data_as(vp), b, a, steps,
                                 out.ctypes.data_as(vp))
        _check(st)
        return out

    def diffuse_counters(self) -> dict:
        """Extension: graph-diffusion calls on this space that passed their checks, the route searches they ran (single or
        batched), the column chunks, the step launches and the seeds uploaded."""
        return _counters(_L.as_diffuse_counters, self._h, ("calls", "route searches", "column chunks", "step launches", "seeds uploaded"))

    @staticmethod
    def _diffuse_solve_params(alpha, tol, max_iters) -> tuple[float, float, int]:
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)):
            raise ValueError(f"max_iters must be an integer in [1, 1024], got {max_iters!r}")
        if not 1 <= max_iters <= 1024:
            raise ValueError(f"max_iters must lie in [1, 1024], got {max_iters}")
        a, t = float(alpha), float(tol)
        if not 0.0 <= a < 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"alpha must lie in [0, 1), got {alpha}")
        if not (np.isfinite(t) and t > 0.0):
            raise ValueError(f"tol must be finite and > 0, got {tol}")
        return a, t, int(max_iters)

    @staticmethod
    def _solve_info_buffers(b: int):
        return np.zeros(b, dtype=np.int32), np.full(b, np.nan, dtype=np.float64), np.zeros(b, dtype=np.int32)

    @staticmethod
    def _solve_info(it, res, stt, single: bool) -> dict:
        """The solve's report: per query the iterations run, sqrt(r.r / b.b) at the stop and whether it converged."""
        if single:
            return {"iterations": int(it[0]), "residual": float(res[0]), "converged": bool(stt[0] == 1)}
        return {"iterations": it.astype(np.int64), "residual": res, "converged": stt == 1}

    def search_diffuse_solve(self, item, gl: GraphLaplacian, tau: float, alpha: float, tol: float = 1e-8, max_iters: int = 100, subset=None,
                             with_info: bool = False):
        """Extension: fixed-point diffusion search -> list[(index, f)] as `search_diffuse` returns it, with the fixed point of
        its recurrence, f = (1 - alpha) (I - alpha S)^-1 y (the manifold-ranking answer), in place of `steps` steps: conjugate
        gradients on the device from x = 0, stopped when |r| <= tol |b| (b = (1 - alpha) y), after `max_iters` iterations, or
        on a breakdown.  About sqrt((1 + alpha) / (1 - alpha)) ln(1 / tol) iterations, each one pass over the graph's CSR and
        streaming passes over four vectors; the arithmetic and the order of every sum are fixed, so f has the bits of the
        numpy reference.  with_info: -> (list, info), info = {"iterations", "residual", "converged"}.  A query that does not
        converge is served with the iterate it has and converged = False; it does not raise.  0 <= alpha < 1, tol finite and
        > 0, 1 <= max_iters <= 1024 (an integer), else ValueError; a feature-mode or row-sharded index raises ValueError."""
        _need_gl(gl)
        q = self._query(item)
        a, t, mi = self._diffuse_solve_params(alpha, tol, max_iters)
        sub = self._as_subset(subset, optional=True)
        n = max(self._hits_bound(gl, sub), 1)
        idx = np.empty(n, dtype=np.int64)
        sc = np.empty(n, dtype=np.float64)
        ln, lq = C.c_int64(0), C.c_double(0.0)
        it, res, stt = self._solve_info_buffers(1)
        st = _L.as_search_diffuse_solve(self._h, gl._h, q.ctypes.data, q.shape[0], float(tau), a, t, mi, _handle(sub), idx.ctypes.data,
                                        sc.ctypes.data, C.byref(ln), C.byref(lq), it.ctypes.data, res.ctypes.data, stt.ctypes.data)
        _check(st)
        out = list(zip(idx[:ln.value].tolist(), sc[:ln.value].tolist()))
        return (out, self._solve_info(it, res, stt, True)) if with_info else out

    def search_batch_diffuse_solve(self, items, gl: GraphLaplacian, tau: float, alpha: float, tol: float = 1e-8, max_iters: int = 100,
                                   subset=None, with_info: bool = False):
        """Extension: batched fixed-point diffusion search, B queries [B, D] -> list of B lists; list i is
        `search_diffuse_solve` over the pool `search_batch` (with a subset: `search_batch_subset`) gives query i.  Every query is
        solved on its own: its f, iteration count and residual do not depend on the others; a query that has stopped is
        frozen while the rest of its chunk of 16 or 64 goes on.  A query whose lambda_q is 0 gets an empty list (0
        iterations, residual NaN, not converged).  with_info: -> (lists, info) with one entry per query."""
        _need_gl(gl)
        Q = _queries_2d(items)
        a, t, mi = self._diffuse_solve_params(alpha, tol, max_iters)
        sub = self._as_subset(subset, optional=True)
        b = Q.shape[0]
        kk = self._hits_bound(gl, sub)
        (idx, sc, ln), stt = _hit_buffers(b, kk), _statuses(b)
        it, res, sst = self._solve_info_buffers(b)
        vp = C.c_void_p
        st = _L.as_search_diffuse_solve_batch(self._h, gl._h, Q.ctypes.data_as(vp), b, Q.shape[1], float(tau), a, t, mi, _handle(sub),
                                              idx.ctypes.data_as(vp), sc.ctypes.data_as(vp), ln.ctypes.data_as(vp), None, stt.ctypes.data_as(vp),
                                              it.ctypes.data_as(vp), res.ctypes.data_as(vp), sst.ctypes.data_as(vp))
        _check(st)
        out = _hit_lists(idx, sc, ln, b, kk)
        return (out, self._solve_info(it, res, sst, False)) if with_info else out

    def score_diffuse_solve(self, item, gl: GraphLaplacian, tau: float, alpha: float, ids, tol: float = 1e-8, max_iters: int = 100,
                            with_info: bool = False):
        """Extension: f of `search_diffuse_solve` (no subset) at the listed ids -> ndarray[float64] of shape (len(ids),), the
        caller's order, duplicates kept.  A query whose lambda_q is 0 panics as `search` does."""
        q = self._query(item)
        out, info = self._score_diffuse_solve(q.reshape(1, -1), gl, tau, alpha, ids, tol, max_iters, True)
        return (out[0], info) if with_info else out[0]

    def score_diffuse_solve_batch(self, items, gl: GraphLaplacian, tau: float, alpha: float, ids, tol: float = 1e-8, max_iters: int = 100,
                                  with_info: bool = False):
        """Extension: f of `search_batch_diffuse_solve` (no subset) at the listed ids -> ndarray[float64] of shape
        (B, len(ids)); a query whose lambda_q is 0 gets a row of NaN, the others are served."""
        out, info = self._score_diffuse_solve(_queries_2d(items), gl, tau, alpha, ids, tol, max_iters, False)
        return (out, info) if with_info else out

    def _score_diffuse_solve(self, Q, gl, tau, alpha, ids, tol, max_iters, single):
        _need_gl(gl)
        a, t, mi = self._diffuse_solve_params(alpha, tol, max_iters)
        ids = _item_ids(ids, self.nitems, "ids")
        b, m = Q.shape[0], ids.shape[0]
        out = np.empty((b, m), dtype=np.float64)
        stt = _statuses(b)
        it, res, sst = self._solve_info_buffers(b)
        vp = C.c_void_p
        st = _L.as_score_diffuse_solve_batch(self._h, gl._h, Q.ctypes.data_as(vp), b, Q.shape[1], float(tau), a, t, mi, ids.ctypes.data_as(vp),
                                             m, out.ctypes.data_as(vp), None, stt.ctypes.data_as(vp), it.ctypes.data_as(vp),
                                             res.ctypes.data_as(vp), sst.ctypes.data_as(vp))
        _check(st, stt if single else None, b)
        return out, self._solve_info(it, res, sst, single)

    def diffuse_solve(self, gl: GraphLaplacian, seeds, alpha: float, tol: float = 1e-8, max_iters: int = 100):
        """Extension: the raw form of the fixed-point solve -> (f, info): f ndarray[float64] of shape (B, nitems), row b the
        solve of `search_diffuse_solve` from the seeds of `seeds[b]` (pairs (ids, values) as `diffuse` takes them), info =
        {"iterations", "residual", "converged"} with one entry per row.  No search, no selection; the whole B x nitems block
        crosses to the host."""
        _need_gl(gl)
        a, t, mi = self._diffuse_solve_params(alpha, tol, max_iters)
        ids, vals, offs = self._diffuse_seeds(seeds, self.nitems)
        b = offs.shape[0] - 1
        out = np.empty((b, self.nitems), dtype=np.float64)
        it, res, sst = self._solve_info_buffers(b)
        vp = C.c_void_p
        st = _L.as_diffuse_solve_seeds(self._h, gl._h, ids.ctypes.data_as(vp), vals.ctypes.data_as(vp), offs.ctypes.data_as(vp), b, a, t, mi,
                                       out.ctypes.data_as(vp), it.ctypes.data_as(vp), res.ctypes.data_as(vp), sst.ctypes.data_as(vp))
        _check(st)
        return out, self._solve_info(it, res, sst, False)

    def diffuse_solve_counters(self) -> dict:
        """Extension: fixed-point diffusion calls on this space that passed their checks, the route searches they ran, the
        column chunks, the iterations launched (per chunk the largest count of its columns), the host's waits and the seeds
        uploaded."""
        return _counters(_L.as_diffuse_solve_counters, self._h,
                         ("calls", "route searches", "column chunks", "iterations launched", "host waits", "seeds uploaded"))

    @staticmethod
    def _eigsh_params(m, tol, max_iters, degree, seed) -> tuple[int, float, int, int, int, int]:
        """The checks of `eigsh` that need no handle -> (m, tol, max_iters, degree, seed, C)."""
        for name, v, lo, hi in (("m", m, 1, 48), ("max_iters", max_iters, 1, 10000), ("degree", degree, 1, 64), ("seed", seed, 0, 2 ** 63 - 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer, got {v!r}")
            if not lo <= v <= hi:
                raise ValueError(f"{name} must lie in [{lo}, {'2^63 - 1' if name == 'seed' else hi}], got {v}")
        t = float(tol)
        if not (np.isfinite(t) and 0.0 < t < 1.0):   # (NaN fails the comparisons)
            raise ValueError(f"tol must be finite and lie in (0, 1), got {tol}")
        return int(m), t, int(max_iters), int(degree), int(seed), 16 if m <= 12 else 64

    def eigsh(self, gl: GraphLaplacian, m: int, tol: float = 1e-8, max_iters: int = 200, degree: int = 16, seed: int = 0,
              with_info: bool = False):
        """Extension: the m largest eigenvalues of the item graph's operator S (the S of `search_diffuse`: the off-diagonal
        entries of the stored Laplacian, negated, i.e. D^-1/2 A D^-1/2) and their eigenvectors -> (values, vectors): values
        ndarray[float64] of shape (m,), descending; vectors of shape (m, nitems), orthonormal, row j belonging to values[j]
        (the layout of the block `diffuse` returns), each with its entry of largest magnitude (lowest index on ties)
        positive.  For rows with an edge, 1 - value is the eigenvalue of the normalised Laplacian: the multiplicity of the
        value 1 is the number of connected components among them, the next value tells the gap (a row without an edge is an
        eigenvector of value 0).  Block Chebyshev-filtered subspace iteration with Rayleigh-Ritz on the device: a block of 16
        columns (m <= 12) or 64, a filter of at most `degree` graph passes per outer iteration, stopped when every wanted
        residual |S v - value v| is <= tol or after `max_iters` outer iterations.  A call that stops at max_iters is served
        with the iterate it has and converged = False; it does not raise.  `seed` picks the start block; the same call
        returns the same bits.  with_info: -> (values, vectors, info), info = {"iterations", "residuals" (m,), "converged",
        "filter_steps" (graph passes launched), "block"}.  1 <= m <= 48, 0 < tol < 1, 1 <= max_iters <= 10000, 1 <= degree <=
        64, 0 <= seed < 2^63 (integers), nitems >= the block's width, and four blocks of nitems x width doubles within the
        "spectral_mib" tuning (default 8192 MiB), else ValueError; a feature-mode or row-sharded index raises ValueError; a
        block that loses a direction (a breakdown) raises RuntimeError."""
        _need_gl(gl)
        m, t, mi, deg, sd, _ = self._eigsh_params(m, tol, max_iters, degree, seed)
        n = self.nitems
        values, vectors, res = np.empty(m, dtype=np.float64), np.empty((m, n), dtype=np.float64), np.empty(m, dtype=np.float64)
        info = np.zeros(4, dtype=np.int64)
        _check(_L.as_graph_eigs(self._h, gl._h, m, t, mi, deg, sd, values.ctypes.data, vectors.ctypes.data, res.ctypes.data, info.ctypes.data))
        if info[1] == 2:
            raise RuntimeError(f"eigsh: the block lost a direction in outer iteration {int(info[0])} (a Gram eigenvalue <= 1e-14 of the largest)")
        if not with_info:
            return values, vectors
        return values, vectors, {"iterations": int(info[0]), "residuals": res, "converged": bool(info[1] == 1), "filter_steps": int(info[2]),
                                 "block": int(info[3])}

    def eigsh_counters(self) -> dict:
        """Extension: `eigsh` calls on this space that passed their checks, their outer iterations, the step (graph pass), Gram
        and rotate launches, and the host's waits (one per Gram, one per residual, one for the answer)."""
        return _counters(_L.as_graph_eigs_counters, self._h,
                         ("calls", "outer iterations", "step launches", "gram launches", "rotate launches", "host waits"))

    _COMPONENTS_KEYS = ("count", "largest", "largest_label", "isolated", "edges_kept", "rounds")

    @staticmethod
    def _components_thresholds(max_dists, single: bool = False) -> np.ndarray:
        """The checks of `components` / `components_sweep` that need no handle -> the thresholds as float64 [T]."""
        what = "max_dist" if single else "max_dists"
        vals = [max_dists] if single else (list(max_dists) if not isinstance(max_dists, (str, bytes)) and np.ndim(max_dists) == 1 else None)
        if vals is None:
            raise ValueError(f"{what} must be a sequence of 1 to 64 numbers, got {max_dists!r}")
        for v in vals:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"{what} must be {'a number' if single else 'numbers'}, got {v!r}")
        if not 1 <= len(vals) <= 64:
            raise ValueError(f"{what} must hold 1 to 64 thresholds, got {len(vals)}")
        t = np.array(vals, dtype=np.float64)
        if np.isnan(t).any():
            raise ValueError(f"{what} must not hold a NaN")
        return t

    def components(self, gl: GraphLaplacian, max_dist=None, with_info: bool = False):
        """Extension: the connected components of the item graph -> labels, ndarray[int32] of shape (nitems,): the label of an
        item is the smallest item id of its component.  The graph's stored entries are used (`gl.to_csr_dist()`): items i and j
        are joined iff the entry i -> j or the entry j -> i is kept, and components are the classes of the transitive closure.
        max_dist None: every stored entry is kept.  max_dist t: an entry is kept iff its dist <= t (a NaN dist never; +inf keeps
        every dist that is no NaN, -inf none) -- the components a build with the same k-NN lists and a smaller eps would connect,
        the single-linkage clusters of the k-NN graph at height t.  An item without a kept entry is its own label.
        with_info: -> (labels, info), info = {"count" (components), "largest" (items of the largest), "largest_label" (the
        smallest label of that size), "isolated" (components of one item), "edges_kept" (stored entries kept, both directions
        as stored), "rounds" (hook-and-compress rounds the device ran)}; all but "rounds" are functions of the graph and t
        alone.  The labels are integers and exact: no tolerance, no dependence on the schedule.  They are valid input to
        `groups(labels)`, and `labels == info["largest_label"]` to `subset(...)`.  A NaN or non-numeric max_dist raises
        ValueError before anything is launched; a feature-mode or row-sharded index raises ValueError."""
        _need_gl(gl)
        t = None if max_dist is None else self._components_thresholds(max_dist, single=True)
        labels = np.empty(max(self.nitems, 1), dtype=np.int32)
        info = np.zeros(6, dtype=np.int64)
        _check(_L.as_graph_components(self._h, gl._h, None if t is None else t.ctypes.data, labels.ctypes.data, info.ctypes.data))
        labels = labels[:self.nitems]
        return (labels, dict(zip(self._COMPONENTS_KEYS, info.tolist()))) if with_info else labels

    def components_sweep(self, gl: GraphLaplacian, max_dists) -> dict:
        """Extension: the statistics of `components(gl, t, with_info=True)` for 1 to 64 thresholds -> a dict with the keys of
        that info, each an ndarray[int64] of shape (T,) in the caller's order (any order, duplicates allowed).  The distinct
        thresholds run in ascending order on the device, each from the labels of the one before (the kept sets are nested),
        from ONE build: which eps connects this data, with no k-NN pass.  No labels cross to the host.  "rounds" of a
        threshold counts the rounds its stage ran from the previous threshold's labels."""
        _need_gl(gl)
        t = self._components_thresholds(max_dists)
        info = np.zeros((t.shape[0], 6), dtype=np.int64)
        _check(_L.as_graph_components_sweep(self._h, gl._h, t.ctypes.data, t.shape[0], info.ctypes.data))
        return {k: info[:, j].copy() for j, k in enumerate(self._COMPONENTS_KEYS)}

    def components_counters(self) -> dict:
        """Extension: `components` / `components_sweep` calls on this space that passed their checks, the thresholds they
        served (1 for a call without one), the hook and compress launches, and the host's waits (one per round, one per
        distinct threshold for the statistics)."""
        return _counters(_L.as_components_counters, self._h, ("calls", "thresholds served", "hook launches", "compress launches", "host waits"))

    def _spectral_op(self, gl: GraphLaplacian, op: str, A, B=None, T=None, coef=None, alias: bool = False):
        """Debug: one S21 primitive on host blocks [n, C] (C = 16 or 64) through the launch `eigsh` makes.  op "step": A = V, B = W
        (None with g == 0), coef = (a, b, g), alias: the result is written over W's block; "gram": A^T B (B None: A^T A) ->
        [C, C]; "rotate": A T with T [C, C]; "colnorm2": the squared column norms of B - A theta with T = theta [C] -> [C]."""
        _need_gl(gl)
        code = {"step": 0, "gram": 1, "rotate": 2, "colnorm2": 3}[op]
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2:
            raise ValueError("argument 'A': expected a 2-D block")
        n, c = A.shape
        same = lambda X, shape: None if X is None else np.ascontiguousarray(X, dtype=np.float64).reshape(shape)   # noqa: E731
        B = same(B, (n, c))
        T = same(T, (c, c) if op == "rotate" else (c,))
        cf = None if coef is None else np.array(list(coef) + [1.0 if alias else 0.0], dtype=np.float64)
        out = np.empty({"step": (n, c), "gram": (c, c), "rotate": (n, c), "colnorm2": (c,)}[op], dtype=np.float64)
        ptr = lambda X: None if X is None else X.ctypes.data   # noqa: E731
        _check(_L.as_spectral_op(self._h, gl._h, code, n, c, ptr(A), ptr(B), ptr(T), ptr(cf), out.ctypes.data))
        return out

    def _lists_args(self, items, gl, lists):
        _need_gl(gl)
        Q = _queries_2d(items)
        ids, offsets = _id_lists(lists, self.nitems)
        if offsets.shape[0] - 1 != Q.shape[0]:
            raise ValueError(f"argument 'lists': {offsets.shape[0] - 1} id lists for {Q.shape[0]} queries")
        return Q, ids, offsets

    def search_batch_lists(self, items, gl: GraphLaplacian, tau: float, lists):
        """Extension: re-ranking of per-query candidate lists, B queries [B, D] EACH WITH ITS OWN id list -> list of B hit
        lists; list i is what `search_subset(items[i], gl, tau, lists[i])` returns: the first min(topk, distinct ids of
        lists[i]) items of that list by (score descending, index ascending) (scores within 1e-12 relative, indices equal
        except inside such ties).  `lists`: a sequence of B id sequences (any order, duplicates allowed, empty lists allowed,
        lists may share ids; a boolean mask of length nitems per list is accepted) or a 2-D integer array (B, C).  Costs one
        `search_batch` over the B queries (lambda_q comes from it; any query whose lambda_q is 0 panics as there, whatever
        its list), then ONE ragged launch on the device scores every (query, item) pair, each query against its own rows,
        and every list is selected there."""
        Q, ids, offsets = self._lists_args(items, gl, lists)
        b = Q.shape[0]
        kk = self._hits_bound(gl)
        (idx, sc, ln), stt = _hit_buffers(b, kk), _statuses(b)
        st = _L.as_search_lists_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau),
                                      ids.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                      idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p),
                                      None, stt.ctypes.data_as(C.c_void_p))
        _check(st, stt, b)
        return _hit_lists(idx, sc, ln, b, kk)

    def score_lists_batch(self, items, gl: GraphLaplacian, tau: float, lists):
        """Extension: scores of per-query candidate lists -> a list of B float64 arrays (a 2-D integer array (B, C) as `lists`
        returns an array (B, C)): entry j of array i is what `score_items(items[i], gl, tau, lists[i])[j]` returns (the
        caller's order, duplicates kept; within 1e-12 relative).  `lists` as for `search_batch_lists`.  Costs one
        `search_batch` over the B queries (lambda_q; a query whose lambda_q is 0 panics as there) plus ONE ragged launch that
        gathers each query's own rows.  The bits of a score depend on its query, its item, tau and lambda_q only: not on the
        entry's position, the other lists, or whether this method or `search_batch_lists` computed it."""
        Q, ids, offsets = self._lists_args(items, gl, lists)
        b = Q.shape[0]
        out = np.empty(ids.shape[0], dtype=np.float64)
        stt = _statuses(b)
        st = _L.as_score_lists_batch(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], float(tau),
                                     ids.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                     out.ctypes.data_as(C.c_void_p), None, stt.ctypes.data_as(C.c_void_p))
        _check(st, stt, b)
        if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.dtype != np.bool_:
            return out.reshape(lists.shape)
        return [out[offsets[i]:offsets[i + 1]] for i in range(b)]

    def lists_counters(self) -> dict:
        """Extension: `search_batch_lists` / `score_lists_batch` calls on this space that passed their checks, the score-kernel
        launches they made, the (query, item) pairs those scored, the lambda_q steps run (`search_batch` calls), and the host
        nanoseconds spent on id checks, deduplication and work tables."""
        return _counters(_L.as_lists_counters, self._h, ("calls", "score_launches", "pairs", "lambda_steps", "host_ns"))

    @staticmethod
    def _taus(taus) -> np.ndarray:
        t = np.ascontiguousarray(taus, dtype=np.float64)
        if t.ndim != 1:
            raise TypeError("argument 'taus': expected a 1-D sequence of floats")
        return t

    def search_batch_lists_taus(self, items, gl: GraphLaplacian, taus, lists):
        """Extension: re-ranking of per-query candidate lists under several taus, B queries [B, D] each with its own id list ->
        for each query a list of one hit list per entry of `taus`; entry [i][j] is what
        `search_batch_lists(items, gl, taus[j], lists)[i]` returns, with the same score bits.  `lists` as for
        `search_batch_lists`.  Costs ONE `search_batch` over the B queries (lambda_q does not depend on tau; a query whose
        lambda_q is 0 panics as there), one upload per chunk of queries and ONE ragged gather per up to 8 distinct taus: every
        cosine is formed once and blended with each tau.  Finite taus only (ValueError otherwise, before anything runs); equal
        taus are computed once; `taus = []` returns B empty lists."""
        Q, ids, offsets = self._lists_args(items, gl, lists)
        t = self._taus(taus)
        b, nt = Q.shape[0], t.shape[0]
        kk = self._hits_bound(gl)
        (idx, sc, ln), stt = _hit_buffers(b * nt, kk), _statuses(b)
        st = _L.as_search_lists_batch_taus(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], t.ctypes.data, nt,
                                           ids.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), idx.ctypes.data,
                                           sc.ctypes.data, ln.ctypes.data, None, stt.ctypes.data)
        _check(st, stt, b)
        return _hit_lists(idx, sc, ln, b * nt, kk, per=nt) if nt else [[] for _ in range(b)]

    def score_lists_batch_taus(self, items, gl: GraphLaplacian, taus, lists):
        """Extension: scores of per-query candidate lists under several taus -> a list of B float64 arrays of shape
        (len(taus), m_i), views of one output buffer (a 2-D integer array (B, C) as `lists` returns an array
        (B, len(taus), C)): row j of array i is what `score_lists_batch(items, gl, taus[j], lists)[i]` returns, with the same
        bits (and the bits `search_batch_lists_taus` gives the same query, tau and item).  Costs one `search_batch` over the B
        queries (lambda_q; a query whose lambda_q is 0 panics as there) and one ragged gather per up to 8 distinct taus.
        `taus = []` returns arrays of shape (0, m_i)."""
        Q, ids, offsets = self._lists_args(items, gl, lists)
        t = self._taus(taus)
        b, nt = Q.shape[0], t.shape[0]
        out = np.empty(nt * ids.shape[0], dtype=np.float64)
        stt = _statuses(b)
        st = _L.as_score_lists_batch_taus(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], t.ctypes.data, nt,
                                          ids.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p), None, stt.ctypes.data)
        _check(st, stt, b)
        if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.dtype != np.bool_:
            return out.reshape(lists.shape[0], nt, lists.shape[1])
        return [out[nt * offsets[i]:nt * offsets[i + 1]].reshape(nt, offsets[i + 1] - offsets[i]) for i in range(b)]

    def lists_sweep_counters(self) -> dict:
        """Extension: `search_batch_lists_taus` / `score_lists_batch_taus` calls on this space that passed their checks, the
        score-kernel launches they made, the (query, item) pairs those gathered (once per launch, not per tau), the (query,
        item, tau) scores they wrote, and the lambda_q steps run (`search_batch` calls)."""
        return _counters(_L.as_lists_sweep_counters, self._h, ("calls", "score_launches", "pairs", "scores", "lambda_steps"))

    def search_subset_taus(self, item, gl: GraphLaplacian, taus, subset):
        """Extension: filtered search under several taus -> one hit list per entry of `taus`, in order; list j is what
        `search_subset(item, gl, taus[j], subset)` returns, with the same score bits.  Costs ONE ordinary `search` (lambda_q
        does not depend on tau; a query whose lambda_q is 0 panics as there) and ONE gather of the subset's rows per up to 8
        distinct taus: every cosine is formed once and blended with each tau.  Every finite tau is served; a NaN or infinite
        one raises ValueError before anything runs; equal taus are computed once; `taus = []` returns `[]`."""
        _need_gl(gl)
        q = self._query(item)
        t = self._taus(taus)
        sub = self._as_subset(subset)
        nt = t.shape[0]
        kk = self._hits_bound(gl, sub)
        idx, sc, ln = _hit_buffers(nt, kk)
        lq = C.c_double(0.0)
        st = _L.as_search_subset_taus(self._h, gl._h, q.ctypes.data, q.shape[0], t.ctypes.data, nt, sub._h, idx.ctypes.data, sc.ctypes.data,
                                      ln.ctypes.data, C.byref(lq))
        _check(st)
        return _hit_lists(idx, sc, ln, nt, kk)

    def score_items_taus(self, item, gl: GraphLaplacian, taus, ids) -> np.ndarray:
        """Extension: re-ranking under several taus -> ndarray[float64] of shape (len(taus), len(ids)): row j is what
        `score_items(item, gl, taus[j], ids)` returns, with the same bits (and the bits `search_subset_taus` gives the same
        tau and item).  Costs one ordinary `search` (lambda_q) and one gather of the listed rows per up to 8 distinct taus."""
        _need_gl(gl)
        q = self._query(item)
        t = self._taus(taus)
        ids = _item_ids(ids, self.nitems, "ids")
        nt, m = t.shape[0], ids.shape[0]
        out = np.empty((nt, m), dtype=np.float64)
        lq = C.c_double(0.0)
        st = _L.as_score_items_taus(self._h, gl._h, q.ctypes.data, q.shape[0], t.ctypes.data, nt, ids.ctypes.data_as(C.c_void_p), m,
                                    out.ctypes.data_as(C.c_void_p), C.byref(lq))
        _check(st)
        return out

    def search_batch_subset_taus(self, items, gl: GraphLaplacian, taus, subset):
        """Extension: batched filtered search under several taus, B queries [B, D] -> for each query a list of one hit list
        per entry of `taus`; entry [i][j] is what `search_batch_subset(items, gl, taus[j], subset)[i]` returns, with the same
        score bits.  Costs ONE `search_batch` over the B queries (lambda_q; a query whose lambda_q is 0 panics as there) and
        one gather of the subset's rows per 64 queries and up to 8 distinct taus (fewer where the score planes would exceed
        the chunk budget).  Finite taus only (ValueError otherwise); equal taus are computed once; `taus = []` returns B empty
        lists."""
        _need_gl(gl)
        Q = _queries_2d(items)
        t = self._taus(taus)
        sub = self._as_subset(subset)
        b, nt = Q.shape[0], t.shape[0]
        kk = self._hits_bound(gl, sub)
        (idx, sc, ln), stt = _hit_buffers(b * nt, kk), _statuses(b)
        st = _L.as_search_subset_batch_taus(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], t.ctypes.data, nt, sub._h,
                                            idx.ctypes.data, sc.ctypes.data, ln.ctypes.data, None, stt.ctypes.data)
        _check(st, stt, b)
        return _hit_lists(idx, sc, ln, b * nt, kk, per=nt) if nt else [[] for _ in range(b)]

    def score_items_batch_taus(self, items, gl: GraphLaplacian, taus, ids) -> np.ndarray:
        """Extension: batched re-ranking under several taus -> ndarray[float64] of shape (B, len(taus), len(ids)): entry
        [i, j] is row i of `score_items_batch(items, gl, taus[j], ids)`, with the same bits.  Costs one `search_batch` over the
        B queries (lambda_q; a query whose lambda_q is 0 panics as there) and one gather of the listed rows per 64 queries and
        up to 8 distinct taus."""
        _need_gl(gl)
        Q = _queries_2d(items)
        t = self._taus(taus)
        ids = _item_ids(ids, self.nitems, "ids")
        b, nt, m = Q.shape[0], t.shape[0], ids.shape[0]
        out = np.empty((b, nt, m), dtype=np.float64)
        stt = _statuses(b)
        st = _L.as_score_items_batch_taus(self._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], t.ctypes.data, nt,
                                          ids.ctypes.data_as(C.c_void_p), m, out.ctypes.data_as(C.c_void_p), None, stt.ctypes.data)
        _check(st, stt, b)
        return out

    def subset_sweep_counters(self) -> dict:
        """Extension: tau sweeps over a subset on this space (all four `*_taus` forms of the filtered search), the score-kernel
        launches they made, the tau planes those launches wrote, and the lambda_q steps run (single searches plus
        `search_batch` calls)."""
        return _counters(_L.as_subset_sweep_counters, self._h, ("calls", "score_launches", "tau_planes", "lambda_steps"))

    def sweep_counters(self) -> dict:
        """Extension: `search_taus` calls on this space, the shared passes that served them, and the taus those passes left
        to the single search (taus_redone)."""
        out = np.zeros(3, dtype=np.int64)
        st = _L.as_sweep_counters(self._h, out.ctypes.data_as(C.c_void_p), 3)
        if st:
            _raise(st)
        return dict(zip(("calls", "shared_passes", "taus_redone"), (int(v) for v in out)))

    def search_batch_taus(self, items, gl: GraphLaplacian, taus):
        """Extension: B queries [B, D] under several taus -> B lists of one hit list per entry of `taus`; entry [b][j] is what
        `search(items[b], gl, taus[j])` returns.  Where `search_batch` batches, the distinct taus in [0, 1] share its batched
        passes (up to 8 per pass: one scan, k-NN step and lambda_q per 32 queries, a scorer tail per (query, tau) pair); equal
        taus are computed once, any other tau takes `search_batch`'s route, and whatever a shared pass does not serve the single
        search."""
        if not isinstance(gl, GraphLaplacian):
            raise TypeError("argument 'gl': expected GraphLaplacian")
        Q = np.ascontiguousarray(items, dtype=np.float64)
        if Q.ndim != 2:
            raise TypeError("items must be a 2-D float64 array")
        t = np.ascontiguousarray(taus, dtype=np.float64)
        if t.ndim != 1:
            raise TypeError("argument 'taus': expected a 1-D sequence of floats")
        b, nt = Q.shape[0], t.shape[0]
        if b == 0:
            return []
        if nt == 0:
            return [[] for _ in range(b)]
        topk = max(min(int(gl.graph_params["topk"]), self.nitems), 0)
        idx = np.empty((b, nt, max(topk, 1)), dtype=np.int64)
        sc = np.empty((b, nt, max(topk, 1)), dtype=np.float64)
        ln = np.zeros((b, nt), dtype=np.int64)
        lq = np.zeros(b, dtype=np.float64)
        stt = np.zeros(b, dtype=np.int32)
        st = _L.as_search_batch_taus(self._h, gl._h, Q.ctypes.data, b, Q.shape[1], t.ctypes.data, nt, idx.ctypes.data, sc.ctypes.data,
                                     ln.ctypes.data, lq.ctypes.data, stt.ctypes.data)
        if st:
            _raise(st)
        if (stt == _lib.AS_EZEROLAMBDA).any():
            raise PanicException("The lambdas are zero, check the magnitude of items and eps.")
        idx, sc = idx[:, :, :topk], sc[:, :, :topk]
        return [[list(zip(ii[:l], ss[:l])) for ii, ss, l in zip(bi, bs, bl)]
                for bi, bs, bl in zip(idx.tolist(), sc.tolist(), ln.tolist())]

    def batch_sweep_counters(self) -> dict:
        """Extension: `search_batch_taus` calls on this space, the batched passes whose scorer tail served them, the (query,
        tau) pairs those passes served, and the pairs they left to the single search (pairs_redone)."""
        out = np.zeros(4, dtype=np.int64)
        st = _L.as_batch_sweep_counters(self._h, out.ctypes.data_as(C.c_void_p), 4)
        if st:
            _raise(st)
        return dict(zip(("calls", "shared_passes", "pairs_served", "pairs_redone"), (int(v) for v in out)))

    def last_search_stats(self) -> dict:
        """Extension: device microseconds of the last search (HIP events on its stream)."""
        out = np.zeros(3, dtype=np.float64)
        st = _L.as_last_search_stats(self._h, out.ctypes.data_as(C.c_void_p), 3)
        if st:
            _raise(st)
        return {"scan_us": out[0], "rest_us": out[1]}

    @property
    def unproven_searches(self) -> int:
        """Extension: searches whose answer failed its a-posteriori exactness check even on the fp64 path (ties inside
        fp64 rounding); the library also says so on stderr the first time.  0 in normal operation."""
        return int(_L.as_unproven_searches(self._h))

    def search_counters(self) -> dict:
        """Extension: what the single-query searches on this space cost so far -- reruns (a second pass over the items) by
        cause, zero-lambda results."""
        out = np.zeros(8, dtype=np.int64)
        st = _L.as_search_counters(self._h, out.ctypes.data_as(C.c_void_p), 8)
        if st:
            _raise(st)
        # (nibble_scans: scans that read the 4-bit tiles; nibble_reruns: those whose search was redone on the 8-bit tiles)
        keys = ("searches", "zero_lambda", "rerun_knn_check", "rerun_overflow", "rerun_score_check", "searches_with_rerun",
                "nibble_scans", "nibble_reruns")
        return dict(zip(keys, (int(v) for v in out)))

    @property
    def knn_pipe(self) -> str:
        """Extension: the matrix pipe the build's k-NN block ran on -- "int8" (two-digit image, the default where the items allow
        it), "bf16" (head + tail), "fp32" (ARROWSPACE_K2_FP32=1) or "none" (feature mode, loaded index)."""
        return {0: "fp32", 1: "bf16", 2: "int8"}.get(int(_L.as_space_knn_pipe(self._h)), "none")

    @property
    def last_scan_int8(self) -> bool:
        """Extension: the last single-query scan read the int8 two-digit image of the items (half the bytes) rather than fp32."""
        return bool(_L.as_last_scan_int8(self._h))

    @property
    def last_scan_operand(self) -> str:
        """Extension: what the last single-query scan read -- "fp32" items, their "int8" two-digit image, or "int8-high" (the
        image's high digits alone: the coarse scan, every candidate re-evaluated exactly)."""
        return {0: "fp32", 1: "int8", 2: "int8-high"}.get(int(_L.as_last_scan_int8(self._h)), "fp32")

    @property
    def last_scan_bits(self) -> int:
        """Extension: width of the coarse operand the last single-query scan read -- 4 for the nibble tiles, 8 otherwise
        (`last_scan_operand` answers "int8-high" for the coarse scan at either width)."""
        return int(_L.as_last_scan_bits(self._h))

    def debug_nibble_image(self):
        """Debugging aid: the nibble tiles as they lie in device memory -- None when the items have no usable image, else a dict
        with `tiles` (uint8 [tile][chunk][64 rows][16 bytes]), `fa4` (the rows' level steps), `r4max` and `chunks`."""
        info = np.zeros(4, dtype=np.float64)
        st = _L.as_debug_nibble_image(self._h, None, 0, None, 0, info.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        if info[0] == 0.0:
            return None
        chunks, rows = int(info[2]), int(info[3])
        tiles = np.zeros((rows // 64, chunks, 64, 16), dtype=np.uint8)
        fa4 = np.zeros(rows, dtype=np.float32)
        st = _L.as_debug_nibble_image(self._h, tiles.ctypes.data_as(C.c_void_p), tiles.nbytes, fa4.ctypes.data_as(C.c_void_p), rows,
                                      info.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        return {"tiles": tiles, "fa4": fa4, "r4max": float(info[1]), "chunks": chunks}

    def debug_i8_image(self):
        """Debugging aid: the int8 two-digit image as it lies in device memory -- None when the items have no usable image, else a
        dict with `x8` (int8 [rows][slab][2][64]: per 64-column slab the high digits a1, then the low digits a2), `fa8` (the rows'
        scales s sqrt(128) / 16256), `x8h` (int8 [tile][chunk][64 rows][16 bytes]: the high digits as the coarse scan reads them),
        `u` and `v` (the maxima the quantiser measured), `coef` (2.001 u + v^2 + 12 * 2^-24), `dp8`, `rows` and `bad`."""
        info = np.zeros(7, dtype=np.float64)
        st = _L.as_debug_i8_image(self._h, None, 0, None, 0, None, 0, info.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        if info[0] == 0.0:
            return None
        dp8, rows = int(info[4]), int(info[5])
        x8 = np.zeros((rows, dp8 // 64, 2, 64), dtype=np.int8)
        fa8 = np.zeros(rows, dtype=np.float32)
        x8h = np.zeros((rows // 64, dp8 // 16, 64, 16), dtype=np.int8)
        st = _L.as_debug_i8_image(self._h, x8.ctypes.data_as(C.c_void_p), x8.nbytes, fa8.ctypes.data_as(C.c_void_p), rows,
                                  x8h.ctypes.data_as(C.c_void_p), x8h.nbytes, info.ctypes.data_as(C.c_void_p))
        if st:
            _raise(st)
        return {"x8": x8, "fa8": fa8, "x8h": x8h, "u": float(info[1]), "v": float(info[2]), "coef": float(info[3]), "dp8": dp8,
                "rows": rows, "bad": int(info[6])}

    def debug_last_dots(self):
        """Debugging aid: the dots the last single-query scan kept (fp32, one per item) and the error coefficient they carry:
        |dot - x.q| <= coef |x||q|."""
        n = int(_L.as_nitems(self._h))
        dots = np.zeros(n, dtype=np.float32)
        coef = C.c_double(0.0)
        st = _L.as_debug_last_dots(self._h, dots.ctypes.data_as(C.c_void_p), n, C.byref(coef))
        if st:
            _raise(st)
        return dots, float(coef.value)

    @property
    def last_batch_int8(self) -> bool:
        """Extension: the last batched pass of `search_batch` ran on the int8 images of items and queries (int8 matrix pipe)."""
        return bool(_L.as_last_batch_int8(self._h))

    @property
    def batch_dual_scans(self) -> int:
        """Extension: scans of `search_batch` that served two passes (64 queries) with one read of the items."""
        return int(_L.as_batch_dual_scans(self._h))

    @property
    def search_pool_size(self) -> int:
        """Extension: single-query workspaces the library holds for this space -- `search` is re-entrant across host threads
        (ctypes releases the GIL around the call), each concurrent call runs on a workspace and stream of its own."""
        return int(_L.as_search_pool_size(self._h))

    def gang_counters(self) -> list:
        """Extension: scans shared by concurrent `search` callers -- [launched with 1 member, 2, 3, 4] (gang scans: host threads whose
        searches arrive together are served by one pass over the items)."""
        out = np.zeros(4, dtype=np.int64)
        st = _L.as_gang_counters(self._h, out.ctypes.data_as(C.c_void_p), 4)
        if st:
            _raise(st)
        return [int(v) for v in out]

    def gang_skips(self) -> dict:
        """Extension: host-prepared single-query scans that did not take the shared path, by first reason."""
        out = np.zeros(10, dtype=np.int64)
        st = _L.as_gang_counters(self._h, out.ctypes.data_as(C.c_void_p), 10)
        if st:
            _raise(st)
        keys = ("no_concurrent_callers", "not_fused_tail", "not_coarse", "state_to_reset", "timed", "row_range")
        return dict(zip(keys, (int(v) for v in out[4:])))

    def save(self, gl: GraphLaplacian, path: str) -> None:
        """Extension: write the built index (items, lambdas, graph) to one file."""
        st = _L.as_index_save(self._h, gl._h, os.fsencode(path))
        if st:
            _raise(st)

    def query_lambda(self, item, gl: GraphLaplacian) -> float:
        """Extension: lambda_q of `prepare_query_item` (src/lib.rs:154) without the search."""
        q = self._query(item)
        topk = min(int(gl.graph_params["topk"]), self.nitems)
        idx = np.empty(max(topk, 1), dtype=np.int64)
        sc = np.empty(max(topk, 1), dtype=np.float64)
        ln, lq = C.c_int64(0), C.c_double(0.0)
        st = _L.as_search(self._h, gl._h, q.ctypes.data_as(C.c_void_p), q.shape[0], 1.0,
                          idx.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(ln), C.byref(lq))
        if st not in (_lib.AS_OK, _lib.AS_EZEROLAMBDA):
            _raise(st)
        return float(lq.value)

    # out of scope: scorer variants whose semantics are not in the tree
    def search_hybrid(self, item, gl, tau):
        raise NotImplementedError("search_hybrid (src/lib.rs:182-219) is outside the hot path built here")

    def search_energy(self, item, gl, k, w_lambda=None, w_dirichlet=None):
        raise NotImplementedError("search_energy (src/lib.rs:232-262) is outside the hot path built here")


class ArrowSpaceBuilder:
    """src/lib.rs:265-377.  The methods are class methods only so that the reference-named module can carry other
    mode defaults (`_mode`); they are called exactly like the reference's static methods."""

    _mode = NORTH_STAR_MODE

    @classmethod
    def build(cls, graph_params, items):
        """(graph_params: dict|None, items: ndarray[float64, 2-D]) -> (ArrowSpace, GraphLaplacian).
        Argument order as the reference (src/lib.rs:271-275)."""
        if not isinstance(items, np.ndarray) or items.dtype != np.float64 or items.ndim != 2:
            raise TypeError("argument 'items': expected a 2-D numpy.ndarray of dtype float64")
        if items.shape[0] == 0 or items.shape[1] == 0:
            raise ValueError("items must be non-empty 2D array")
        gp, op = _parse_graph_params(graph_params, cls._mode)
        esz = items.itemsize
        rs, cs = items.strides[0] // esz, items.strides[1] // esz
        if items.strides[0] % esz or items.strides[1] % esz or rs < 0 or cs < 0:
            items = np.ascontiguousarray(items)
            rs, cs = items.shape[1], 1
        sp, gr = C.c_void_p(), C.c_void_p()
        st = _L.as_build(items.ctypes.data_as(C.c_void_p), items.shape[0], items.shape[1], rs, cs, C.byref(gp),
                         C.byref(op), C.byref(sp), C.byref(gr))
        if st:
            _raise(st)
        return ArrowSpace._wrap(sp), GraphLaplacian._wrap(gr)

    @classmethod
    def build_from_device(cls, graph_params, data_ptr: int, dtype, n: int, d: int, ld: int | None = None):
        """Extension: items already resident in HBM (row-major fp32 or fp64 at `data_ptr`,
        e.g. `torch_tensor.data_ptr()`); same result as build() on the same values."""
        gp, op = _parse_graph_params(graph_params, cls._mode)
        dt = {"float32": _lib.DTYPE_F32, "float64": _lib.DTYPE_F64}[str(dtype).replace("torch.", "")]
        sp, gr = C.c_void_p(), C.c_void_p()
        st = _L.as_build_dev(C.c_void_p(int(data_ptr)), dt, int(n), int(d), int(ld if ld is not None else d),
                             C.byref(gp), C.byref(op), C.byref(sp), C.byref(gr))
        if st:
            _raise(st)
        return ArrowSpace._wrap(sp), GraphLaplacian._wrap(gr)

    @staticmethod
    def load(path: str):
        """Extension: (ArrowSpace, GraphLaplacian) from a file written by ArrowSpace.save()."""
        op = Opts()
        op.device = int(os.environ.get("ARROWSPACE_DEVICE", "-1"))
        sp, gr = C.c_void_p(), C.c_void_p()
        st = _L.as_index_load(os.fsencode(path), C.byref(op), C.byref(sp), C.byref(gr))
        if st:
            _raise(st)
        return ArrowSpace._wrap(sp), GraphLaplacian._wrap(gr)

    @staticmethod
    def build_energy(items, energy_params=None, graph_params=None):
        raise NotImplementedError("build_energy (src/lib.rs:333-376) is outside the hot path built here")
