"""GPU: the grow-only work buffers of the filtered, list and range searches, reused across forms.  A subset handle keeps ONE set
of buffers (query stage, scores, selection scratch) for its single-query, batched and tau-sweep calls, the space keeps one for
`score_items*` and one for the list forms; every call may find them sized by an earlier call of another form.  Each answer of a
long-lived handle is compared bit for bit (indices, scores, lengths) with the same call on a handle that has served nothing
else.

A subset handle has a fixed id list, so the sequence runs on two long-lived handles side by side: m = 600 (the selection is the
one-block sort alone) and m = 1500 (m > SUBSET_TOPK: the radix select).  The handle whose m does change between calls is the
space's own (`score_items*`): it is compared with a second space built from the same items that sees the calls in reverse order.
"""
import numpy as np
import pytest

from conftest import calibrate_eps, clustered
from test_gpu_subset_batch import draw_queries, raw_batch

pytestmark = pytest.mark.gpu

N, D, TOPK, TAU = 3000, 40, 10, 0.62   # (d = 40: the padded query row is longer than the query)
TAUS3 = [0.1, 0.62, 1.0]
TAUS11 = [0.0, 0.05, 0.1, 0.2, 0.3, 0.45, 0.62, 0.7, 0.8, 0.9, 1.0]   # two groups of the single sweep: 8 + 3


@pytest.fixture(scope="module")
def world():
    import pyarrowspace_amd as asp
    X = np.ascontiguousarray(clustered(N, D, nclust=24, seed=41).astype(np.float32).astype(np.float64))
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": TOPK, "p": 2.0, "sigma": None}
    a, gl_a = asp.ArrowSpaceBuilder.build(gp, X)
    b, gl_b = asp.ArrowSpaceBuilder.build(gp, X)
    assert np.array_equal(a.lambdas(), b.lambdas())
    rng = np.random.default_rng(42)
    Q, _ = draw_queries(a, gl_a, X, rng, 70)
    Qz = Q.copy()
    Qz[37] = 50.0   # no item within eps: lambda_q == 0, in the middle of the first chunk of 64
    ids = {m: np.sort(rng.choice(N, m, replace=False)) for m in (600, 1500)}
    return asp, a, gl_a, b, gl_b, Q, np.ascontiguousarray(Qz), ids, rng


def raw_scores(asp, space, gl, Q, tau, ids):
    """as_score_items_batch through the C ABI: (status, scores with unwritten entries at -5, per-query status)."""
    b = Q.shape[0]
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    out = np.full((b, len(ids)), -5.0)
    lq, stt = np.zeros(b), np.zeros(b, dtype=np.int32)
    st = asp._L.as_score_items_batch(space._h, gl._h, Q.ctypes.data, b, Q.shape[1], float(tau), ids.ctypes.data, len(ids), out.ctypes.data,
                                     lq.ctypes.data, stt.ctypes.data)
    return st, out, stt.tolist()


def test_one_handle_serves_every_form_like_a_fresh_one(world):
    asp, a, gl, _, _, Q, Qz, ids, _ = world
    held = {m: a.subset(v) for m, v in ids.items()}
    q0, Q3, Q5 = np.ascontiguousarray(Q[0]), np.ascontiguousarray(Q[:3]), np.ascontiguousarray(Q[:5])

    def same(m, call):
        """`call(subset)` on the long-lived handle of m ids and on a fresh one"""
        got, want = call(held[m]), call(a.subset(ids[m]))
        assert got == want
        return got

    def raw70(sub):
        st, lists, lq, stt, ln = raw_batch(asp, a, gl, Qz, TAU, sub, TOPK)
        assert st == 0 and stt[37] == asp._lib.AS_EZEROLAMBDA and ln[37] == 0 and (np.delete(ln, 37) == TOPK).all()
        return lists, lq.tolist(), stt.tolist(), ln.tolist()

    try:
        # single searches: the sort alone, the radix select, the sort again
        first = same(600, lambda s: a.search_subset(q0, gl, TAU, s))
        assert len(first) == TOPK
        same(1500, lambda s: a.search_subset(q0, gl, TAU, s))
        assert same(600, lambda s: a.search_subset(q0, gl, TAU, s)) == first
        # batched: one tile; two chunks under a 1 MiB budget (64 + 6 queries of 1500 scores), a zero-lambda query inside the first; one tile
        small = {}
        for m in (1500, 600):
            small[m] = same(m, lambda s: a.search_batch_subset(Q3, gl, TAU, s))
            assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
            same(m, raw70)
            assert asp._L.as_set_tuning(b"subset_batch_mib", 0) == 0
            assert same(m, lambda s: a.search_batch_subset(Q3, gl, TAU, s)) == small[m]
        # tau sweeps: one group, two groups, the batched sweep; then the first single search
        for m in (1500, 600):
            same(m, lambda s: a.search_subset_taus(q0, gl, TAUS3, s))
            same(m, lambda s: a.search_subset_taus(q0, gl, TAUS11, s))
            same(m, lambda s: a.search_batch_subset_taus(Q5, gl, TAUS11, s))
        assert same(600, lambda s: a.search_subset(q0, gl, TAU, s)) == first
        same(1500, lambda s: a.search_subset(q0, gl, TAU, s))
        # range search on the same handle: an append buffer of 64 entries overflows and the compaction runs again
        sc = a.score_items_batch(Q5, gl, TAU, ids[1500])
        thr = float(np.sort(sc.ravel())[-300])
        before = a.range_counters()["relaunches"]
        assert asp._L.as_set_tuning(b"range_cap", 64) == 0
        tight = same(1500, lambda s: a.search_range_batch(Q5, gl, TAU, thr, s))
        assert a.range_counters()["relaunches"] >= before + 2   # (the held and the fresh handle)
        assert asp._L.as_set_tuning(b"range_cap", 0) == 0
        assert same(1500, lambda s: a.search_range_batch(Q5, gl, TAU, thr, s)) == tight
        assert 300 <= sum(len(h) for h in tight) <= 310   # (more than 300 only if scores tie at the threshold)
        # ... and the handle still searches
        assert same(1500, lambda s: a.search_batch_subset(Q3, gl, TAU, s)) == small[1500]
        same(1500, lambda s: a.search_subset(q0, gl, TAU, s))
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 0) == 0
        assert asp._L.as_set_tuning(b"range_cap", 0) == 0


def test_the_spaces_own_buffers_serve_every_form(world):
    """`score_items*` (all scores, no selection) on the space's own work buffers, whose id count changes from call to call, and the
    list forms on theirs: space `a` runs the calls in this order, space `b` (the same items) in the reverse order."""
    asp, a, gl_a, b, gl_b, Q, Qz, ids, rng = world
    q0, Q3, Q5 = np.ascontiguousarray(Q[0]), np.ascontiguousarray(Q[:3]), np.ascontiguousarray(Q[:5])

    def lists_of(per):
        r = np.random.default_rng(per)
        return [r.choice(N, per, replace=False) for _ in range(5)]

    def batch70(s, g):
        st, out, stt = raw_scores(asp, s, g, Qz, TAU, ids[1500])
        assert st == 0 and stt[37] == asp._lib.AS_EZEROLAMBDA and (out[37] == -5.0).all() and (np.delete(out, 37, 0) != -5.0).all()
        return out.tolist()

    def tuned(key, v, call):
        def run(s, g):
            assert asp._L.as_set_tuning(key, v) == 0
            try:
                return call(s, g)
            finally:
                assert asp._L.as_set_tuning(key, 0) == 0
        return run

    calls = [
        lambda s, g: s.score_items(q0, g, TAU, ids[600]).tolist(),
        lambda s, g: s.score_items(q0, g, TAU, ids[1500]).tolist(),
        lambda s, g: s.score_items(q0, g, TAU, ids[600]).tolist(),
        lambda s, g: s.score_items_batch(Q3, g, TAU, ids[1500]).tolist(),
        tuned(b"subset_batch_mib", 1, batch70),
        lambda s, g: s.score_items_batch(Q3, g, TAU, ids[600]).tolist(),
        lambda s, g: s.score_items_taus(q0, g, TAUS3, ids[1500]).tolist(),
        lambda s, g: s.score_items_taus(q0, g, TAUS11, ids[1500]).tolist(),
        lambda s, g: s.score_items_batch_taus(Q5, g, TAUS11, ids[1500]).tolist(),
        lambda s, g: s.score_items_batch(Q5, g, TAU, ids[1500]).tolist(),   # the k == 0 route after the sweeps
        lambda s, g: s.score_items(q0, g, TAU, ids[600]).tolist(),
        # the list forms: 200 entries, 5000, 200 again, then the tau sweep
        lambda s, g: s.search_batch_lists(Q5, g, TAU, lists_of(40)),
        lambda s, g: s.search_batch_lists(Q5, g, TAU, lists_of(1000)),
        lambda s, g: s.search_batch_lists(Q5, g, TAU, lists_of(40)),
        lambda s, g: s.search_batch_lists_taus(Q5, g, TAUS11, lists_of(1000)),
    ]
    try:
        got = [c(a, gl_a) for c in calls]
        want = [c(b, gl_b) for c in reversed(calls)][::-1]
        for i, (x, y) in enumerate(zip(got, want)):
            assert x == y, f"call {i}"
        assert got[0] == got[2] == got[10] and got[11] == got[13]
        # the selecting and the all-scores routes give one (query, item) pair the same bits
        hits = a.search_batch_subset(Q3, gl_a, TAU, ids[1500])
        pos = {int(j): t for t, j in enumerate(ids[1500])}
        for i, h in enumerate(hits):
            assert [s for _, s in h] == [got[3][i][pos[j]] for j, _ in h]
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 0) == 0


def test_handles_come_and_go(world):
    """20 handles made, used for a batched call and dropped: every one answers alike."""
    asp, a, gl, _, _, Q, _, ids, _ = world
    Q3 = np.ascontiguousarray(Q[:3])
    want = a.search_batch_subset(Q3, gl, TAU, ids[1500])
    for _ in range(20):
        sub = a.subset(ids[1500])
        assert a.search_batch_subset(Q3, gl, TAU, sub) == want
        del sub
