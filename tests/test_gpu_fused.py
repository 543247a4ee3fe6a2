"""GPU: fused multi-query search -- ArrowSpace.search_fused / score_fused: ONE answer to J query vectors, the
weighted sum or the largest weighted term of their S11 scores, folded on the device.  Expected values: the route there was
before -- `score_items_batch` of the same ids folded by the numpy reference tests/fused_ref.py and ordered by lexsort (equality of
indices and of score bits, no tolerance) -- and the fp64 oracle's per-vector scores folded by the same reference (the project's
own bounds, scaled by the weights).  Shapes and recipe: tests/test_gpu_range.py's."""
import os
import sys

import numpy as np
import pytest

import fused_ref
from conftest import assert_hits_match, calibrate_eps, clustered
from test_gpu_parity import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TAU = 0.62
# (n, d, k, topk, metric, kernel, rounded through float32)
SHAPES = {"1200x48": (1200, 48, 10, 10, "l2", "gaussian", False), "1500x51": (1500, 51, 8, 6, "l2", "gaussian", False),
          "700x768f32": (700, 768, 12, 15, "l2", "gaussian", True), "3000x96cos": (3000, 96, 25, 10, "cosine", "rational", False)}
JS = (1, 2, 5, 64, 65)   # 64: the score kernel's query tile; 65: one past it
MODES = ("sum", "max")
NVEC = 130               # served query vectors kept per shape: three chunks of 64 under a one-MiB budget
_built = {}


def atol_for(d):
    """fp64 dot error of unit-norm rows: scores at tau = 1 can sit near 0, where a relative bound means nothing."""
    return 16 * d * 2.0 ** -53


def index(name):
    """One index per shape for the whole module: (asp, X, graph parameters, aspace, gl, NVEC query vectors whose lambda_q is
    not 0: the query recipe of test_gpu_subset.py)."""
    if name not in _built:
        import pyarrowspace_amd as asp
        n, d, k, topk, metric, kernel, f32 = SHAPES[name]
        X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
        if f32:
            X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
        gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        rng = np.random.default_rng(n)
        vecs = []
        while len(vecs) < NVEC:
            q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
            if aspace.query_lambda(q, gl) != 0.0:
                vecs.append(q)
        _built[name] = (asp, X, gp, aspace, gl, np.stack(vecs))
    return _built[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def weights_of(J, rng):
    """(name, what the caller passes, what the reference folds with)."""
    rnd = rng.uniform(-1.0, 1.0, J)
    neg = np.full(J, 1.0 / J)
    neg[J // 2] = -0.75
    return [("default", None, np.full(J, 1.0 / J)), ("random", rnd, rnd), ("one negative", neg, neg)]


def subsets_of(n, topk, rng):
    """(name, ids ascending or None for every item)."""
    return [("none", None), ("257 ids", np.sort(rng.choice(n, 257, replace=False))), ("one id", np.array([int(rng.integers(0, n))])),
            ("M <= topk", np.sort(rng.choice(n, max(topk - 2, 2), replace=False)))]


def check_both_forms(aspace, gl, Q, ids, handle, S, passed, w, mode, topk, **kw):
    """`score_fused` and `search_fused` against the fold of S ([J, len(ids)], the scores of `ids`) under weights w."""
    F = fused_ref.fuse(S, w, mode)
    got = aspace.score_fused(Q, gl, TAU, ids, weights=passed, mode=mode, **kw)
    assert got.dtype == np.float64 and got.shape == F.shape and bits(got) == bits(F)
    wi, ws = fused_ref.top(ids, F, topk)
    hits = aspace.search_fused(Q, gl, TAU, weights=passed, mode=mode, subset=handle, **kw)
    assert len(hits) == min(topk, len(ids))
    assert [i for i, _ in hits] == wi.tolist()
    assert bits([v for _, v in hits]) == bits(ws)
    return hits


@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_against_the_route_there_was_before(name, J):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(1000 + J)
    Q = V[:J]
    for sname, ids in subsets_of(n, gp["topk"], rng):
        handle = None if ids is None else aspace.subset(ids)
        ids = np.arange(n) if ids is None else ids
        S = aspace.score_items_batch(Q, gl, TAU, ids)
        assert not np.isnan(S).any()
        for wname, passed, w in weights_of(J, rng):
            for mode in MODES:
                check_both_forms(aspace, gl, Q, ids, handle, S, passed, w, mode, gp["topk"])
        # the score form keeps the caller's order and duplicates; the ad-hoc subset forms give the prepared handle's answer
        if len(ids) > 2:
            mixed = np.concatenate([ids[::-1][:40], ids[:3], ids[:3]])
            w = weights_of(J, rng)[1][2]
            pos = np.searchsorted(ids, mixed)
            got = aspace.score_fused(Q, gl, TAU, mixed, weights=w)
            assert bits(got) == bits(fused_ref.fuse(S[:, pos], w, "sum"))
            if handle is not None:
                want = aspace.search_fused(Q, gl, TAU, weights=w, subset=handle)
                assert aspace.search_fused(Q, gl, TAU, weights=w, subset=ids[::-1].copy()) == want
                assert aspace.search_fused(Q, gl, TAU, weights=w, subset=ids.tolist()) == want


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_accumulator_carries_across_chunks(name):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(2)
    J = NVEC
    Q = V[:J]
    ids = np.arange(n)
    S = aspace.score_items_batch(Q, gl, TAU, ids)
    per_chunk = min(max((1 << 20) // (8 * n) // 64 * 64, 64), 4096)   # queries whose scores fit one MiB, in tiles of 64
    chunks = -(-J // per_chunk)
    # 64 queries a chunk wherever a row of scores is longer than 8 KiB: three chunks, the last of 2 rows (700 items: 128 + 2)
    assert chunks == (2 if name == "700x768f32" else 3)
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
        for wname, passed, w in weights_of(J, rng):
            for mode in MODES:
                c0 = aspace.fused_counters()
                check_both_forms(aspace, gl, Q, ids, None, S, passed, w, mode, gp["topk"])
                c1 = aspace.fused_counters()
                # two calls: `chunks` launches and J x n scores folded each, one lambda_q step each
                assert c1[1] - c0[1] == 2 * chunks and c1[2] - c0[2] == 2 * J * n and c1[3] - c0[3] == 2 and c1[0] - c0[0] == 2
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    c0 = aspace.fused_counters()
    check_both_forms(aspace, gl, Q, ids, None, S, None, np.full(J, 1.0 / J), "sum", gp["topk"])
    assert aspace.fused_counters()[1] - c0[1] == 2   # one chunk under the default budget


@pytest.mark.parametrize("name", list(SHAPES))
def test_consequences_of_s13(name):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(3)
    some = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(some)
    q = V[7]
    for ids, handle, listed in ((np.arange(n), None, np.arange(n)), (some, sub, some)):
        topk = min(gp["topk"], len(ids))
        single = aspace.search_batch_subset(q[None, :], gl, TAU, listed)[0]
        for mode in MODES:
            # J = 1, w = [1.0]: the batched filtered form's list, bit for bit
            got = aspace.search_fused(q[None, :], gl, TAU, weights=[1.0], mode=mode, subset=handle)
            assert [i for i, _ in got] == [i for i, _ in single]
            assert bits([v for _, v in got]) == bits([v for _, v in single])
            assert aspace.search_fused(q[None, :], gl, TAU, mode=mode, subset=handle) == got   # the default weight of J = 1 is 1.0
        # (q, q) with (+1, -1) under sum: F = +0.0 everywhere, the first topk ids of the subset
        got = aspace.search_fused(np.stack([q, q]), gl, TAU, weights=[1.0, -1.0], mode="sum", subset=handle)
        assert [i for i, _ in got] == ids[:topk].tolist()
        assert bits([v for _, v in got]) == bits(np.zeros(topk))
        assert bits(aspace.score_fused(np.stack([q, q]), gl, TAU, ids, weights=[1.0, -1.0])) == bits(np.zeros(len(ids)))
        # max over J copies of one vector with w = 1: the J = 1 answer
        want = aspace.search_fused(q[None, :], gl, TAU, weights=[1.0], mode="max", subset=handle)
        for J in (2, 5):
            got = aspace.search_fused(np.stack([q] * J), gl, TAU, weights=np.ones(J), mode="max", subset=handle)
            assert [i for i, _ in got] == [i for i, _ in want] and bits([v for _, v in got]) == bits([v for _, v in want])


@pytest.mark.parametrize("name", ["1200x48", "3000x96cos"])
def test_zero_lambda(name):
    asp, X, gp, aspace, gl, V = index(name)
    n, d = X.shape
    rng = np.random.default_rng(4)
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0 (the recipe of test_gpu_diverse.py)
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, TAU)
    ids = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(ids)
    w = np.array([0.5, -0.25, 0.75, 0.4, 0.3])

    def counted(call, exc=None):
        c0 = aspace.fused_counters()
        if exc is None:
            out = call()
        else:
            with pytest.raises(exc):
                call()
            out = None
        c1 = aspace.fused_counters()
        assert c1[3] - c0[3] == 1, (c0, c1)
        if exc is not None:
            assert c1[1] == c0[1]   # a call that panics folds nothing
        return out

    for at in (0, 2, 4):
        Q = V[10:15].copy()
        Q[at] = far
        others = np.array([t for t in range(5) if t != at])
        for mode in MODES:
            for passed, wref in ((w, w), (None, np.full(5, 0.2))):
                for handle, listed in ((None, np.arange(n)), (sub, ids)):
                    counted(lambda: aspace.search_fused(Q, gl, TAU, weights=passed, mode=mode, subset=handle), asp.PanicException)
                    counted(lambda: aspace.score_fused(Q, gl, TAU, listed, weights=passed, mode=mode), asp.PanicException)
                    # skip: the answer over the other vectors with their own weights, not renormalised
                    got = counted(lambda: aspace.search_fused(Q, gl, TAU, weights=passed, mode=mode, subset=handle, on_zero_lambda="skip"))
                    want = aspace.search_fused(Q[others], gl, TAU, weights=wref[others], mode=mode, subset=handle)
                    assert [i for i, _ in got] == [i for i, _ in want] and bits([v for _, v in got]) == bits([v for _, v in want])
                    got = counted(lambda: aspace.score_fused(Q, gl, TAU, listed, weights=passed, mode=mode, on_zero_lambda="skip"))
                    assert bits(got) == bits(aspace.score_fused(Q[others], gl, TAU, listed, weights=wref[others], mode=mode))
    # every vector far: the panic under both settings, an empty subset included
    Qf = np.stack([far, far * 1.5, far])
    for ozl in ("raise", "skip"):
        for handle in (None, sub, []):
            counted(lambda: aspace.search_fused(Qf, gl, TAU, subset=handle, on_zero_lambda=ozl), asp.PanicException)
        counted(lambda: aspace.score_fused(Qf, gl, TAU, ids, on_zero_lambda=ozl), asp.PanicException)
        counted(lambda: aspace.score_fused(Qf[:1], gl, TAU, [], mode="max", on_zero_lambda=ozl), asp.PanicException)


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_fp64_oracle(oracle_lib, name):
    asp, X, gp, aspace, gl, V = index(name)
    n, d = X.shape
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(5)
    some = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(some)
    vecs, rows = [], []
    for q in V:   # per-vector oracle scores, as test_gpu_range.py obtains them
        try:
            _, lq = ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            continue
        vecs.append(q)
        rows.append(ref.scores(q, TAU, lq))
        if len(vecs) == 8:
            break
    assert len(vecs) == 8
    for J in (3, 8):
        Q, S = np.stack(vecs[:J]), np.stack(rows[:J])
        mixed = rng.uniform(0.2, 1.0, J) * np.where(np.arange(J) % 2 == 0, 1.0, -1.0)
        for w in (rng.uniform(0.2, 1.0, J), mixed):
            for mode in MODES:
                F = fused_ref.fuse(S, w, mode)
                for ids, handle in ((np.arange(n), None), (some, sub)):
                    wi, ws = fused_ref.top(ids, F[ids], gp["topk"])
                    got = aspace.search_fused(Q, gl, TAU, weights=w, mode=mode, subset=handle)
                    assert_hits_match(got, list(zip(wi.tolist(), ws.tolist())), all_scores=F, rtol=RTOL, atol=float(np.abs(w).sum()) * atol_for(d))
                    np.testing.assert_allclose(aspace.score_fused(Q, gl, TAU, ids, weights=w, mode=mode), F[ids], rtol=RTOL,
                                               atol=float(np.abs(w).sum()) * atol_for(d))


def test_errors_on_the_device_path():
    asp, X, gp, aspace, gl, V = index("1200x48")
    n, d = X.shape
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    Q = V[:3]
    sub = aspace.subset([1, 2, 3])
    wide = np.ascontiguousarray(np.concatenate([Q, np.ones((3, 1))], axis=1))
    cases = ((ValueError, "another space", lambda: other.search_fused(Q, gl2, TAU, subset=sub)),
             (ValueError, "query length", lambda: aspace.search_fused(wide, gl, TAU)),
             (ValueError, "query length", lambda: aspace.search_fused(wide, gl, TAU, subset=sub, mode="max")),
             (ValueError, "query length", lambda: aspace.score_fused(wide, gl, TAU, [0, 1])),
             (ValueError, "tau", lambda: aspace.search_fused(Q, gl, float("nan"))),
             (ValueError, "tau", lambda: aspace.search_fused(Q, gl, float("inf"), subset=sub)),
             (ValueError, "tau", lambda: aspace.score_fused(Q, gl, float("nan"), [0, 1], mode="max")),
             (ValueError, "id", lambda: aspace.score_fused(Q, gl, TAU, [0, n])),
             (ValueError, "id", lambda: aspace.search_fused(Q, gl, TAU, subset=[0, n])))
    for exc, match, call in cases:
        c0, o0 = aspace.fused_counters(), other.fused_counters()
        with pytest.raises(exc, match=match):
            call()
        assert aspace.fused_counters() == c0 and other.fused_counters() == o0   # nothing was launched, no lambda_q step either
    # the C ABI's own refusals: j <= 0, a mode other than 0 / 1, a weight that is not finite
    import ctypes as C
    idx, sc, ln = np.zeros(16, dtype=np.int64), np.zeros(16), C.c_int64(5)
    for j, wts, mode, what in ((0, None, 0, "j must be"), (-1, None, 0, "j must be"), (3, None, 2, "mode"), (3, None, -1, "mode"),
                               (3, np.array([1.0, np.nan, 1.0]), 0, "finite"), (3, np.array([1.0, 1.0, -np.inf]), 1, "finite")):
        c0 = aspace.fused_counters()
        st = asp._L.as_search_fused(aspace._h, gl._h, Q.ctypes.data, j, d, TAU, None if wts is None else wts.ctypes.data, mode, 0, None,
                                    idx.ctypes.data, sc.ctypes.data, C.byref(ln), None, None)
        assert st == asp._lib.AS_EINVAL and what in asp._lib.last_error() and ln.value == 0
        assert aspace.fused_counters() == c0
    # an empty subset and an empty id list: an empty answer, but the lambda_q step runs
    for s in (aspace.subset([]), [], np.zeros(n, dtype=bool)):
        c0 = aspace.fused_counters()
        assert aspace.search_fused(Q, gl, TAU, subset=s) == []
        c1 = aspace.fused_counters()
        assert c1[3] - c0[3] == 1 and c1[1] == c0[1]
    c0 = aspace.fused_counters()
    out = aspace.score_fused(Q, gl, TAU, [])
    assert out.shape == (0,) and out.dtype == np.float64
    c1 = aspace.fused_counters()
    assert c1[3] - c0[3] == 1 and c1[1] == c0[1]
    # the neighbours on a handle are undisturbed
    before = aspace.search_subset(Q[0], gl, TAU, sub)
    aspace.search_fused(Q, gl, TAU, subset=sub)
    assert aspace.search_subset(Q[0], gl, TAU, sub) == before
