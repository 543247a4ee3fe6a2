"""GPU: range search -- ArrowSpace.search_range / count_range / search_range_batch / count_range_batch: EVERY item of a subset
whose S11 score is >= a threshold, by (score descending, index ascending).  Expected values: `score_items` / `score_items_batch`
of the same ids filtered and ordered by numpy (equality of indices and of score bits, no tolerance), and the fp64 oracle's
scores at thresholds that sit in a gap between two of them (equality of the id sets)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from conftest import calibrate_eps, clustered
from test_gpu_parity import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

INF = float("inf")
# (n, d, k, topk, metric, kernel, rounded through float32)
SHAPES = {"1200x48": (1200, 48, 10, 10, "l2", "gaussian", False), "1500x51": (1500, 51, 8, 6, "l2", "gaussian", False),
          "700x768f32": (700, 768, 12, 15, "l2", "gaussian", True), "3000x96cos": (3000, 96, 25, 10, "cosine", "rational", False)}
RANKS = (1, 5, 64, 65, 257)   # a partial wave, one wave + 1, one block + 1; m // 2 and the last element are added per subset
_built = {}


def atol_for(d):
    """fp64 dot error of unit-norm rows: scores at tau = 1 can sit near 0, where a relative bound means nothing."""
    return 16 * d * 2.0 ** -53


def index(name):
    """One index per shape for the whole module: (asp, X, graph parameters, aspace, gl)."""
    if name not in _built:
        import pyarrowspace_amd as asp
        n, d, k, topk, metric, kernel, f32 = SHAPES[name]
        X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
        if f32:
            X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
        gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        _built[name] = (asp, X, gp, aspace, gl)
    return _built[name]


def queries_of(X, rng, count, aspace=None, gl=None):
    """The query recipe of test_gpu_subset.py; with an index, only queries whose lambda_q is not 0."""
    n, d = X.shape
    out = []
    while len(out) < count:
        q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
        if aspace is None or aspace.query_lambda(q, gl) != 0.0:
            out.append(q)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def expected(ids, s, thr):
    """{(i, s[i]) : s[i] >= thr} by (score descending, index ascending): numpy's IEEE >= and lexsort."""
    keep = s >= thr
    i, v = ids[keep], s[keep]
    order = np.lexsort((i, -v))
    return i[order].tolist(), v[order]


def check_exact(got, ids, s, thr):
    wi, ws = expected(ids, s, thr)
    assert [i for i, _ in got] == wi, (thr, len(got), len(wi))
    assert bits([v for _, v in got]) == bits(ws), thr
    return len(wi)


def subsets_of(n, rng):
    mask = rng.random(n) < 0.3
    return [("none", None, np.arange(n)), ("half", None, np.sort(rng.choice(n, n // 2, replace=False))),
            ("one percent", None, np.sort(rng.choice(n, max(n // 100, 1), replace=False))),
            ("one id", None, np.array([int(rng.integers(0, n))])), ("ends", None, np.array([0, n - 1])),
            ("mask", mask, np.flatnonzero(mask))]


def thresholds_of(s):
    """-inf, +inf, just above the maximum, the exact r-th largest score (equality is included) and the next double above it
    (the r-th item is excluded): [(threshold, r or None, excluded)]."""
    m = len(s)
    ss = np.sort(s)[::-1]
    out = [(-INF, None, False), (INF, None, False), (np.nextafter(ss[0], INF), None, False)]
    for r in sorted({r for r in RANKS + (m // 2, m) if 1 <= r <= m}):
        out.append((float(ss[r - 1]), r, False))
        out.append((float(np.nextafter(ss[r - 1], INF)), r, True))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_and_membership_against_score_items(name):
    asp, X, gp, aspace, gl = index(name)
    n, d = X.shape
    rng = np.random.default_rng(7)
    q = queries_of(X, rng, 1, aspace, gl)[0]
    subs = subsets_of(n, rng)
    prepared = {nm: (None if nm == "none" else aspace.subset(ids if raw is None else raw)) for nm, raw, ids in subs}
    for tau in (1.0, 0.62, 0.0):
        for nm, raw, ids in subs:
            s = aspace.score_items(q, gl, tau, ids)
            assert not np.isnan(s).any()
            order = np.lexsort((ids, -s))
            for thr, r, excluded in thresholds_of(s):
                got = aspace.search_range(q, gl, tau, thr, prepared[nm])
                cnt = check_exact(got, ids, s, thr)
                assert aspace.count_range(q, gl, tau, thr, prepared[nm]) == cnt == len(got)
                if thr == -INF:
                    assert cnt == len(ids)
                elif r is None:
                    assert cnt == 0
                elif excluded:
                    assert int(ids[order[r - 1]]) not in {i for i, _ in got} and cnt < r
                else:
                    assert cnt >= r and got[r - 1] == (int(ids[order[r - 1]]), float(s[order[r - 1]]))
            # the ad-hoc forms of the same subset: an array, a list, a mask
            thr = float(np.sort(s)[::-1][min(4, len(s) - 1)])
            want = aspace.search_range(q, gl, tau, thr, prepared[nm])
            if nm != "none":
                assert aspace.search_range(q, gl, tau, thr, ids[::-1].copy()) == want
                assert aspace.search_range(q, gl, tau, thr, ids.tolist()) == want
            if raw is not None:
                assert aspace.search_range(q, gl, tau, thr, raw) == want
                assert aspace.count_range(q, gl, tau, thr, raw) == len(want)


@pytest.mark.parametrize("name", list(SHAPES))
def test_sets_against_the_oracle_at_thresholds_inside_a_gap(oracle_lib, name):
    asp, X, gp, aspace, gl = index(name)
    n, d = X.shape
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(7)
    Q = queries_of(X, rng, 3)
    half = np.sort(rng.choice(n, n // 2, replace=False))
    sub = aspace.subset(half)
    checked = 0
    for q in Q:
        try:
            _, lq = ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            continue
        checked += 1
        for tau in (1.0, 0.62):
            sc = ref.scores(q, tau, lq)
            ss = np.sort(sc)[::-1]
            for r0 in (1, 5, 64, 65, 257, n // 2, n - 1):
                r = r0
                while r < n - 1 and (ss[r - 1] - ss[r]) < 1e-7 * max(abs(ss[r - 1]), abs(ss[r])):
                    r += 1
                assert r - r0 <= 64 and (ss[r - 1] - ss[r]) >= 1e-7 * max(abs(ss[r - 1]), abs(ss[r])), (r0, r)
                thr = 0.5 * (ss[r - 1] + ss[r])
                for ids, handle in ((np.arange(n), None), (half, sub)):
                    got = aspace.search_range(q, gl, tau, thr, handle)
                    want = ids[sc[ids] >= thr]
                    assert sorted(i for i, _ in got) == want.tolist(), (r, tau)
                    gi = np.array([i for i, _ in got], dtype=np.int64)
                    np.testing.assert_allclose([v for _, v in got], sc[gi], rtol=RTOL, atol=atol_for(d))
                    assert aspace.count_range(q, gl, tau, thr, handle) == len(want)
    assert checked >= 2


def counters(asp, aspace):
    out = (C.c_int64 * 6)()
    assert asp._L.as_range_counters(aspace._h, out, 6) == 0
    return list(out)


def test_overflow_of_the_append_buffer_relaunches_the_compaction_only():
    asp, X, gp, aspace, gl = index("1200x48")
    n, d = X.shape
    rng = np.random.default_rng(11)
    q = queries_of(X, rng, 1, aspace, gl)[0]
    tau = 0.62
    ids = np.arange(n)
    s = aspace.score_items(q, gl, tau, ids)
    ss = np.sort(s)[::-1]
    cases = [(thr, int((s >= thr).sum())) for thr in (float(np.nextafter(ss[0], INF)), float(ss[6]), float(ss[7]), float(ss[1100]))]
    assert [t for _, t in cases[:3]] == [0, 7, 8] and cases[3][1] > 1000
    sub = aspace.subset(np.arange(0, n, 2))
    base = [(aspace.search_range(q, gl, tau, thr, None), aspace.search_range(q, gl, tau, thr, sub)) for thr, _ in cases]
    for (thr, total), (full, _) in zip(cases, base):
        assert check_exact(full, ids, s, thr) == total
    try:
        assert asp._L.as_set_tuning(b"range_cap", 7) == 0
        for (thr, total), (full, part) in zip(cases, base):
            c0 = counters(asp, aspace)
            got = aspace.search_range(q, gl, tau, thr, None)
            c1 = counters(asp, aspace)
            assert got == full and bits([v for _, v in got]) == bits([v for _, v in full])
            assert c1[4] - c0[4] == (1 if total > 7 else 0), (total, c0, c1)
            assert c1[1] - c0[1] == (2 if total > 7 else 1) and c1[0] - c0[0] == 1 and c1[5] - c0[5] == 1
            assert c1[2] - c0[2] == n and c1[3] - c0[3] == total
            assert aspace.count_range(q, gl, tau, thr, None) == total
            c2 = counters(asp, aspace)
            assert c2[4] == c1[4] and c2[1] - c1[1] == 1 and c2[3] - c1[3] == total
            # a prepared subset has buffers of its own: the same path there
            got = aspace.search_range(q, gl, tau, thr, sub)
            c3 = counters(asp, aspace)
            assert got == part and c3[4] - c2[4] == (1 if len(part) > 7 else 0)
    finally:
        assert asp._L.as_set_tuning(b"range_cap", 0) == 0
    for (thr, total), (full, _) in zip(cases, base):
        assert aspace.search_range(q, gl, tau, thr, None) == full


def same_but_for_threshold_ties(batched, single, thr, tie=1e-12):
    """A batched list against the single form's: scores within `tie` relative, the same ids except for items whose score lies
    within `tie` relative of the threshold."""
    b, s = dict(batched), dict(single)
    for i in set(b) ^ set(s):
        v = b[i] if i in b else s[i]
        assert abs(v - thr) <= tie * abs(thr), (i, v, thr)
    common = sorted(set(b) & set(s))
    np.testing.assert_allclose([b[i] for i in common], [s[i] for i in common], rtol=tie, atol=0.0)


@pytest.mark.parametrize("nb", [1, 3, 65, 130])
@pytest.mark.parametrize("name", ["1500x51", "700x768f32"])
def test_batched_forms(name, nb):
    asp, X, gp, aspace, gl = index(name)
    n, d = X.shape
    rng = np.random.default_rng(100 + nb)
    Q = np.stack(queries_of(X, rng, nb, aspace, gl))
    tau = 0.62
    half = np.sort(rng.choice(n, n // 2, replace=False))
    one = np.array([int(rng.integers(0, n))])
    for ids, handle in ((np.arange(n), None), (half, aspace.subset(half)), (one, aspace.subset(one))):
        S = aspace.score_items_batch(Q, gl, tau, ids)
        m = len(ids)
        # one threshold per query: the exact value of one of its own scores; with three or more queries an -inf and an +inf
        thr = np.array([np.sort(S[i])[::-1][min((7 * i) % 90, m - 1)] for i in range(nb)])
        if nb >= 3:
            thr[1], thr[2] = -INF, INF
        got = aspace.search_range_batch(Q, gl, tau, thr, handle)
        assert len(got) == nb
        for i in range(nb):
            check_exact(got[i], ids, S[i], thr[i])
        if nb >= 3:
            assert len(got[1]) == m and got[2] == []
        cnt = aspace.count_range_batch(Q, gl, tau, thr, handle)
        assert cnt.dtype == np.int64 and cnt.tolist() == [len(g) for g in got]
        # a scalar threshold serves every query
        t0 = float(np.median(np.sort(S, axis=1)[:, -min(20, m)]))
        flat = aspace.search_range_batch(Q, gl, tau, t0, handle)
        for i in range(nb):
            check_exact(flat[i], ids, S[i], t0)
        assert aspace.count_range_batch(Q, gl, tau, t0, handle).tolist() == [len(g) for g in flat]
        # against the single form
        for i in sorted({0, nb // 2, nb - 1}):
            same_but_for_threshold_ties(got[i], aspace.search_range(Q[i], gl, tau, float(thr[i]), handle), thr[i])
        # several chunks of queries, and an append buffer that overflows in every chunk: the same answer
        try:
            assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
            assert aspace.search_range_batch(Q, gl, tau, thr, handle) == got
            assert asp._L.as_set_tuning(b"range_cap", 7) == 0
            c0 = counters(asp, aspace)
            again = aspace.search_range_batch(Q, gl, tau, thr, handle)
            c1 = counters(asp, aspace)
            assert again == got and all(bits([v for _, v in a]) == bits([v for _, v in g]) for a, g in zip(again, got))
            chunks = (c1[1] - c0[1]) - (c1[4] - c0[4])
            per_chunk = min(max((1 << 20) // (8 * m) // 64 * 64, 64), 4096)   # queries whose scores fit one MiB, in tiles of 64
            assert chunks == -(-nb // per_chunk) and (chunks >= 2 or nb < 130 or m < n)
            if sum(len(g) for g in got) > 7 * chunks:
                assert c1[4] > c0[4]
            assert aspace.count_range_batch(Q, gl, tau, thr, handle).tolist() == [len(g) for g in got]
            assert counters(asp, aspace)[4] == c1[4]
        finally:
            assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
            assert asp._L.as_set_tuning(b"range_cap", 0) == 0


def test_errors_and_edges():
    asp, X, gp, aspace, gl = index("1200x48")
    n, d = X.shape
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    near = np.ascontiguousarray(X[3] * 1.01)
    far = np.ascontiguousarray(np.full(d, 50.0))   # no item within eps: lambda_q == 0
    Qn = np.stack([near, near * 1.01])
    sub = aspace.subset([1, 2, 3])
    empty = aspace.subset([])
    assert aspace.query_lambda(near, gl) != 0.0
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, 1.0)
    # thresholds
    for call in (lambda: aspace.search_range(near, gl, 0.62, float("nan")), lambda: aspace.count_range(near, gl, 0.62, float("nan"), sub),
                 lambda: aspace.search_range(near, gl, 0.62, [0.5, 0.5]), lambda: aspace.search_range_batch(Qn, gl, 0.62, [0.5, float("nan")]),
                 lambda: aspace.search_range_batch(Qn, gl, 0.62, [0.5]), lambda: aspace.count_range_batch(Qn, gl, 0.62, [0.5, 0.5, 0.5]),
                 lambda: aspace.search_range_batch(Qn, gl, 0.62, [[0.5, 0.5]])):
        c0 = counters(asp, aspace)
        with pytest.raises(ValueError):
            call()
        assert counters(asp, aspace) == c0   # nothing was launched
    with pytest.raises(TypeError):
        aspace.search_range(near, gl, 0.62, "0.5")
    with pytest.raises(TypeError):
        aspace.search_range_batch(Qn, gl, 0.62, ["a", "b"])
    # the C ABI refuses a NaN threshold itself
    h = C.c_void_p(1)
    assert asp._L.as_search_range(aspace._h, gl._h, near.ctypes.data, d, 0.62, float("nan"), None, 0, C.byref(h), None) == asp._lib.AS_EINVAL
    assert h.value is None and "NaN" in asp._lib.last_error()
    # the filtered forms' checks and messages
    with pytest.raises(ValueError, match="query length"):
        aspace.search_range(np.ascontiguousarray(near[:10]), gl, 0.62, 0.5)
    with pytest.raises(ValueError, match="query length"):
        aspace.count_range_batch(np.ascontiguousarray(Qn[:, :10]), gl, 0.62, 0.5, sub)
    with pytest.raises(ValueError, match="another space"):
        other.search_range(np.ascontiguousarray(X[3] * 1.01), gl2, 0.62, 0.5, sub)
    with pytest.raises(ValueError, match="another space"):
        other.search_range_batch(Qn, gl2, 0.62, 0.5, sub)
    with pytest.raises(ValueError, match="tau"):
        aspace.search_range(near, gl, float("nan"), 0.5, sub)
    with pytest.raises(ValueError, match="tau"):
        aspace.count_range_batch(Qn, gl, float("inf"), 0.5)
    with pytest.raises(ValueError, match="id"):
        aspace.search_range(near, gl, 0.62, 0.5, [0, n])
    with pytest.raises(TypeError):
        aspace.search_range(near, None, 0.62, 0.5)
    with pytest.raises(TypeError):
        aspace.search_range_batch(Qn, None, 0.62, 0.5)
    with pytest.raises(TypeError):
        aspace.search_range(near.astype(np.float32), gl, 0.62, 0.5)
    # lambda_q == 0 panics whatever the subset and the threshold, in all four forms
    Qf = np.stack([near, far, near])
    for s in (None, sub, empty, []):
        for thr in (0.5, INF):
            with pytest.raises(asp.PanicException):
                aspace.search_range(far, gl, 0.62, thr, s)
            with pytest.raises(asp.PanicException):
                aspace.count_range(far, gl, 0.62, thr, s)
            with pytest.raises(asp.PanicException):
                aspace.search_range_batch(Qf, gl, 0.62, thr, s)
            with pytest.raises(asp.PanicException):
                aspace.count_range_batch(Qf, gl, 0.62, thr, s)
    # the C ABI serves the other queries of such a batch
    thr3 = np.full(3, -INF)
    st = np.full(3, 9, dtype=np.int32)
    lq = np.full(3, -1.0)
    h = C.c_void_p()
    assert asp._L.as_search_range_batch(aspace._h, gl._h, Qf.ctypes.data, 3, d, 0.62, thr3.ctypes.data, sub._h, 0, C.byref(h), lq.ctypes.data,
                                        st.ctypes.data) == 0
    try:
        offs = np.zeros(4, dtype=np.int64)
        assert asp._L.as_range_queries(h) == 3 and asp._L.as_range_offsets(h, offs.ctypes.data) == 0
        assert offs.tolist() == [0, 3, 3, 6] and asp._L.as_range_total(h) == 6
        assert st.tolist() == [0, asp._lib.AS_EZEROLAMBDA, 0] and lq[1] == 0.0 and lq[0] == pytest.approx(aspace.query_lambda(near, gl), rel=1e-9)
        idx = np.zeros(6, dtype=np.int64)
        sc = np.zeros(6)
        assert asp._L.as_range_copy(h, idx.ctypes.data, sc.ctypes.data) == 0
        assert sorted(idx[:3].tolist()) == [1, 2, 3] and sorted(idx[3:].tolist()) == [1, 2, 3]
    finally:
        asp._L.as_range_free(h)
    # count_only answers hold no entries
    h = C.c_void_p()
    assert asp._L.as_search_range(aspace._h, gl._h, near.ctypes.data, d, 0.62, -INF, sub._h, 1, C.byref(h), None) == 0
    try:
        assert asp._L.as_range_total(h) == 3 and asp._L.as_range_queries(h) == 1
        idx = np.zeros(3, dtype=np.int64)
        sc = np.zeros(3)
        assert asp._L.as_range_copy(h, idx.ctypes.data, sc.ctypes.data) == asp._lib.AS_EINVAL
    finally:
        asp._L.as_range_free(h)
    # an empty subset: no answer, but the lambda_q step runs
    for s in (empty, [], np.zeros(n, dtype=bool)):
        c0 = counters(asp, aspace)
        assert aspace.search_range(near, gl, 0.62, -INF, s) == []
        assert aspace.count_range(near, gl, 0.62, -INF, s) == 0
        assert aspace.search_range_batch(Qn, gl, 0.62, -INF, s) == [[], []]
        assert aspace.count_range_batch(Qn, gl, 0.62, -INF, s).tolist() == [0, 0]
        c1 = counters(asp, aspace)
        assert c1[5] - c0[5] == 4 and c1[0] - c0[0] == 4 and c1[1] == c0[1]
    # B == 0 launches nothing
    c0 = counters(asp, aspace)
    Q0 = np.empty((0, d))
    assert aspace.search_range_batch(Q0, gl, 0.62, 0.5) == []
    assert aspace.search_range_batch(Q0, gl, 0.62, [], sub) == []
    cnt = aspace.count_range_batch(Q0, gl, 0.62, 0.5)
    assert cnt.shape == (0,) and cnt.dtype == np.int64
    c1 = counters(asp, aspace)
    assert c1[5] == c0[5] and c1[1] == c0[1]
    # the answer is not cut at topk, and +-inf are thresholds like any other
    full = aspace.search_range(near, gl, 0.62, -INF)
    assert len(full) == n > gp["topk"] and aspace.search_range(near, gl, 0.62, INF) == []
    assert full[:gp["topk"]] == aspace.search_subset(near, gl, 0.62, np.arange(n))


def test_the_neighbours_on_a_handle_are_undisturbed_and_threads_get_the_serial_answers():
    asp, X, gp, aspace, gl = index("3000x96cos")
    n, d = X.shape
    rng = np.random.default_rng(21)
    ids_a, ids_b = np.sort(rng.choice(n, 1500, replace=False)), np.sort(rng.choice(n, 900, replace=False))
    sub_a, sub_b = aspace.subset(ids_a), aspace.subset(ids_b)
    Q = queries_of(X, rng, 8, aspace, gl)
    tau = 0.62
    before = [(aspace.search_subset(q, gl, tau, sub_a), bits(aspace.score_items(q, gl, tau, ids_a))) for q in Q]
    thr = [float(np.sort(aspace.score_items(q, gl, tau, ids_a))[::-1][40]) for q in Q]
    serial_a = [aspace.search_range(q, gl, tau, t, sub_a) for q, t in zip(Q, thr)]
    serial_b = [aspace.search_range(q, gl, tau, t, sub_b) for q, t in zip(Q, thr)]
    serial_all = [aspace.search_range(q, gl, tau, t) for q, t in zip(Q, thr)]
    assert all(len(s) >= 41 for s in serial_a)
    aspace.search_range_batch(np.stack(Q), gl, tau, thr, sub_a)
    aspace.count_range(Q[0], gl, tau, -INF, sub_a)
    after = [(aspace.search_subset(q, gl, tau, sub_a), bits(aspace.score_items(q, gl, tau, ids_a))) for q in Q]
    assert after == before
    errors = []

    def run(handle, want):
        try:
            for q, t, w in zip(Q, thr, want):
                assert aspace.search_range(q, gl, tau, t, handle) == w
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    for pair in (((sub_a, serial_a), (sub_a, serial_a)), ((sub_a, serial_a), (sub_b, serial_b)), ((None, serial_all), (None, serial_all))):
        th = [threading.Thread(target=run, args=a) for a in pair]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors[0]
    assert [(aspace.search_subset(q, gl, tau, sub_a), bits(aspace.score_items(q, gl, tau, ids_a))) for q in Q] == before
