"""GPU: batched fused search -- ArrowSpace.search_fused_batch / score_fused_batch: B needs of J_b query vectors
each in one call, every need folded into an accumulator row of its own on the device.  Expected values: `score_items_batch` over
the call's flattened vectors, folded need by need by the numpy reference tests/fused_batch_ref.py and ordered by lexsort (equality
of indices and of score bits, no tolerance); the single forms for B = 1; the fp64 oracle's per-vector scores folded by the same
reference (section 5.16's bounds).  Shapes, recipe and indexes: tests/test_gpu_fused.py's (one index per shape for the session)."""
import ctypes as C

import numpy as np
import pytest

import fused_ref
from conftest import assert_hits_match
from fused_batch_ref import default_weights, fuse_batch
from test_gpu_fused import MODES, SHAPES, TAU, atol_for, bits, index, subsets_of, weights_of
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

RAGGED = (1, 2, 5, 64, 65, 3, 130, 1)   # a need cut by a chunk edge (64-row chunks), one over three chunks, J = 1 at both ends
ON_EDGES = (64, 1, 63, 128, 3)          # needs that start exactly on the edges 64, 128 and 256
_vectors = {}


def vectors(name, count):
    """`count` distinct query vectors of the shape whose lambda_q is not 0: test_gpu_fused.py's, then more by its recipe."""
    asp, X, gp, aspace, gl, V = index(name)
    have = _vectors.get(name, V)
    if have.shape[0] < count:
        n, d = X.shape
        rng = np.random.default_rng(7 * n + 1)
        more = []
        while have.shape[0] + len(more) < count:
            q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
            if aspace.query_lambda(q, gl) != 0.0:
                more.append(q)
        have = _vectors[name] = np.concatenate([have, np.stack(more)])
    return have[:count]


def split(V, Js):
    """(needs: a list of (J_b, D) arrays cut from V in order, offsets)."""
    offs = np.concatenate([[0], np.cumsum(Js)]).astype(np.int64)
    return [V[offs[b]:offs[b + 1]] for b in range(len(Js))], offs


def need_weights(Js, which, rng):
    """weights_of per need -> (what the caller passes, the flattened weights the reference folds with)."""
    per = [weights_of(J, rng)[which] for J in Js]
    passed = None if which == 0 else [p for _, p, _ in per]
    return passed, np.concatenate([w for _, _, w in per])


def tuning(asp, key, value):
    assert asp._L.as_set_tuning(key, value) == 0


def check_both_forms(aspace, gl, needs, offs, ids, handle, S, passed, wflat, mode, topk, served=None, **kw):
    """`score_fused_batch` and `search_fused_batch` against the need-by-need fold of S ([sum J, len(ids)]) under wflat."""
    F = fuse_batch(S, offs, wflat, mode, served)
    got = aspace.score_fused_batch(needs, gl, TAU, ids, weights=passed, mode=mode, **kw)
    assert got.dtype == np.float64 and got.shape == (len(needs), len(ids)) and bits(got) == bits(F)
    hits = aspace.search_fused_batch(needs, gl, TAU, weights=passed, mode=mode, subset=handle, **kw)
    assert len(hits) == len(needs)
    for b in range(len(needs)):
        if served is not None and not any(served[offs[b]:offs[b + 1]]):
            assert hits[b] == []
            continue
        wi, ws = fused_ref.top(ids, F[b], topk)
        assert len(hits[b]) == min(topk, len(ids))
        assert [i for i, _ in hits[b]] == wi.tolist(), b
        assert bits([v for _, v in hits[b]]) == bits(ws), b
    return got, hits


@pytest.mark.parametrize("Js", [RAGGED, ON_EDGES], ids=["ragged", "on edges"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_ragged_needs_across_tile_and_chunk_edges(name, Js):
    asp, X, gp, aspace, gl, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(1500 + len(Js))
    V = vectors(name, sum(Js))
    needs, offs = split(V, Js)
    cases = []
    for sname, ids in subsets_of(n, gp["topk"], rng):
        handle = None if ids is None else aspace.subset(ids)
        ids = np.arange(n) if ids is None else ids
        S = aspace.score_items_batch(V, gl, TAU, ids)   # the reference's scores, under the default budget
        assert not np.isnan(S).any()
        cases.append((sname, ids, handle, S))
    try:
        tuning(asp, b"subset_batch_mib", 1)
        for sname, ids, handle, S in cases:
            for which in range(3):
                passed, wflat = need_weights(Js, which, rng)
                for mode in MODES:
                    c0 = aspace.fused_batch_counters()
                    check_both_forms(aspace, gl, needs, offs, ids, handle, S, passed, wflat, mode, gp["topk"])
                    c1 = aspace.fused_batch_counters()
                    d = {k: c1[k] - c0[k] for k in c1}
                    assert d["calls"] == 2 and d["needs"] == 2 * len(Js) and d["lambda_steps"] == 2 and d["groups"] == 2
                    assert d["folded"] == 2 * sum(Js) * len(ids)
                    if name == "1200x48" and sname == "none":
                        # 64 rows a chunk: ceil(sum J / 64) launches a call
                        assert d["launches"] == 2 * -(-sum(Js) // 64)
    finally:
        tuning(asp, b"subset_batch_mib", 256)


@pytest.mark.parametrize("name", ["1200x48", "1500x51"])
def test_the_answer_does_not_depend_on_the_need_groups(name):
    asp, X, gp, aspace, gl, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(16)
    Js = RAGGED
    V = vectors(name, sum(Js))
    needs, offs = split(V, Js)
    some = np.sort(rng.choice(n, 257, replace=False))
    for ids, handle in ((np.arange(n), None), (some, aspace.subset(some))):
        S = aspace.score_items_batch(V, gl, TAU, ids)
        row = 8 * len(ids)   # bytes of an accumulator row
        # KiB budgets (negative values) that hold exactly one and exactly two rows; the default holds every need
        one, two = -(-row // 1024), -(-2 * row // 1024)
        assert row <= one * 1024 < 2 * row and 2 * row <= two * 1024 < 3 * row
        seen = []
        try:
            for setting, groups in ((-one, len(Js)), (-two, -(-len(Js) // 2)), (0, 1)):
                tuning(asp, b"fused_batch_mib", setting)
                for mode in MODES:
                    passed, wflat = need_weights(Js, 1, np.random.default_rng(17))
                    c0 = aspace.fused_batch_counters()
                    got, hits = check_both_forms(aspace, gl, needs, offs, ids, handle, S, passed, wflat, mode, gp["topk"])
                    c1 = aspace.fused_batch_counters()
                    assert c1["groups"] - c0["groups"] == 2 * groups and c1["lambda_steps"] - c0["lambda_steps"] == 2
                    seen.append((mode, bits(got), hits))
        finally:
            tuning(asp, b"fused_batch_mib", 0)
        for mode, b, h in seen:
            first = next(s for s in seen if s[0] == mode)
            assert b == first[1] and h == first[2]


@pytest.mark.parametrize("name", ["1200x48", "1500x51"])
def test_later_loop_trips_return_the_same_bits(name):
    asp, X, gp, aspace, gl, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(18)
    Js = (3, 1, 9, 2)
    V = vectors(name, sum(Js))
    needs, offs = split(V, Js)
    # 257 ids: an odd m in one block; 1199 ids: an odd m whose single last position falls into the third trip under a cap of 1
    for ids in (np.arange(n), np.sort(rng.choice(n, 257, replace=False)), np.sort(rng.choice(n, 1199, replace=False))):
        handle = aspace.subset(ids)
        S = aspace.score_items_batch(V, gl, TAU, ids)
        passed, wflat = need_weights(Js, 1, rng)
        for mode in MODES:
            want = check_both_forms(aspace, gl, needs, offs, ids, handle, S, passed, wflat, mode, gp["topk"])
            try:
                for cap in (1, 3):
                    tuning(asp, b"filtered_grid_cap", cap)
                    got = check_both_forms(aspace, gl, needs, offs, ids, handle, S, passed, wflat, mode, gp["topk"])
                    assert bits(got[0]) == bits(want[0]) and got[1] == want[1]
            finally:
                tuning(asp, b"filtered_grid_cap", 0)


@pytest.mark.parametrize("J", [1, 2, 65])
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_need_is_the_single_form_bit_for_bit(name, J):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(19 + J)
    Q = V[20:20 + J]
    some = np.sort(rng.choice(n, 257, replace=False))
    for ids, handle in ((np.arange(n), None), (some, aspace.subset(some))):
        for wname, passed, w in weights_of(J, rng):
            for mode in MODES:
                want = aspace.search_fused(Q, gl, TAU, weights=passed, mode=mode, subset=handle)
                got = aspace.search_fused_batch(Q[None], gl, TAU, weights=None if passed is None else [passed], mode=mode, subset=handle)
                assert len(got) == 1 and [i for i, _ in got[0]] == [i for i, _ in want]
                assert bits([v for _, v in got[0]]) == bits([v for _, v in want])
                wantF = aspace.score_fused(Q, gl, TAU, ids, weights=passed, mode=mode)
                gotF = aspace.score_fused_batch([Q], gl, TAU, ids, weights=None if passed is None else passed[None], mode=mode)
                assert gotF.shape == (1, len(ids)) and bits(gotF[0]) == bits(wantF)
        if J == 1:   # therefore: J = 1 with weight [1.0] is the batched filtered form's list
            single = aspace.search_batch_subset(Q, gl, TAU, ids)[0]
            for mode in MODES:
                got = aspace.search_fused_batch(Q[None], gl, TAU, weights=[[1.0]], mode=mode, subset=handle)[0]
                assert [i for i, _ in got] == [i for i, _ in single] and bits([v for _, v in got]) == bits([v for _, v in single])


@pytest.mark.parametrize("name", list(SHAPES))
def test_plus_and_minus_one_cancel_to_positive_zero_between_ordinary_needs(name):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(20)
    some = np.sort(rng.choice(n, 257, replace=False))
    q = V[7]
    needs = [V[30:33], np.stack([q, q]), V[40:42]]
    weights = [None, [1.0, -1.0], [0.25, -2.0]]
    wflat = np.array([1.0 / 3] * 3 + [1.0, -1.0] + [0.25, -2.0])
    Vf, offs = np.concatenate(needs), np.array([0, 3, 5, 7])
    for ids, handle in ((np.arange(n), None), (some, aspace.subset(some))):
        topk = min(gp["topk"], len(ids))
        S = aspace.score_items_batch(Vf, gl, TAU, ids)
        got, hits = check_both_forms(aspace, gl, needs, offs, ids, handle, S, weights, wflat, "sum", gp["topk"])
        assert bits(got[1]) == bits(np.zeros(len(ids)))
        assert [i for i, _ in hits[1]] == ids[:topk].tolist() and bits([v for _, v in hits[1]]) == bits(np.zeros(topk))
        # the neighbours are what they are alone in a call of the same vectors' scores: no accumulator row leaks into another
        assert bits(got[0]) == bits(fused_ref.fuse(S[0:3], wflat[0:3], "sum")) and bits(got[2]) == bits(fused_ref.fuse(S[5:7], wflat[5:7], "sum"))
        assert np.abs(got[0]).max() > 0.0 and np.abs(got[2]).max() > 0.0


def per_vector_scores(asp, aspace, gl, V, ids):
    """The rows `score_items_batch` writes for V where some lambda_q may be 0 (the C entry leaves such a row unwritten and
    reports it; the Python method panics) -> (S with NaN in those rows, served flags)."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    S = np.full((V.shape[0], len(ids)), np.nan)
    stt = np.zeros(V.shape[0], dtype=np.int32)
    st = asp._L.as_score_items_batch(aspace._h, gl._h, V.ctypes.data_as(C.c_void_p), V.shape[0], V.shape[1], float(TAU),
                                     ids.ctypes.data_as(C.c_void_p), len(ids), S.ctypes.data_as(C.c_void_p), None,
                                     stt.ctypes.data_as(C.c_void_p))
    assert st == 0
    return S, (stt != asp._lib.AS_EZEROLAMBDA).tolist()


@pytest.mark.parametrize("name", ["1200x48", "3000x96cos"])
def test_zero_lambda(name):
    asp, X, gp, aspace, gl, V = index(name)
    n, d = X.shape
    rng = np.random.default_rng(21)
    far = np.full(d, 50.0)   # no item within eps (the recipe of test_gpu_fused.py)
    assert aspace.query_lambda(far, gl) == 0.0 and aspace.query_lambda(far * 1.5, gl) == 0.0
    some = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(some)
    needs = [V[50:53], np.stack([V[53], far, V[54]]), np.stack([far, far * 1.5]), V[55:57], np.stack([far, V[57]]), np.stack([V[58], far * 1.5])]
    Vf, offs = np.concatenate(needs), np.array([0, 3, 6, 8, 10, 12, 14])
    want_served = [True] * 3 + [True, False, True] + [False, False] + [True, True] + [False, True] + [True, False]
    weights = [None, [0.5, -0.25, 0.75], None, [0.4, 0.3], None, [2.0, 1.0]]
    wflat = np.array([1.0 / 3] * 3 + [0.5, -0.25, 0.75] + [0.5, 0.5] + [0.4, 0.3] + [0.5, 0.5] + [2.0, 1.0])

    def counted(call, exc=None):
        c0 = aspace.fused_batch_counters()
        if exc is None:
            out = call()
        else:
            with pytest.raises(exc):
                call()
            out = None
        c1 = aspace.fused_batch_counters()
        assert c1["lambda_steps"] - c0["lambda_steps"] == 1 and c1["calls"] - c0["calls"] == 1, (c0, c1)
        return out, c1["launches"] - c0["launches"]

    for ids, handle in ((np.arange(n), None), (some, sub)):
        S, served = per_vector_scores(asp, aspace, gl, Vf, ids)
        assert served == want_served
        for mode in MODES:
            for passed, wref in ((weights, wflat), (None, default_weights(offs))):
                # raise: the panic of the whole call, nothing folded
                for call in (lambda: aspace.search_fused_batch(needs, gl, TAU, weights=passed, mode=mode, subset=handle),
                             lambda: aspace.score_fused_batch(needs, gl, TAU, ids, weights=passed, mode=mode)):
                    assert counted(call, asp.PanicException)[1] == 0
                # skip: the served vectors of each need with their own weights; need 2 has none left
                got, hits = check_both_forms(aspace, gl, needs, offs, ids, handle, S, passed, wref, mode, gp["topk"], served=served,
                                             on_zero_lambda="skip")
                assert hits[2] == [] and np.isnan(got[2]).all() and not np.isnan(got[[0, 1, 3, 4, 5]]).any()
                # the needs without such a vector keep the bits they have in a call of their own vectors' scores
                assert bits(got[0]) == bits(fused_ref.fuse(S[0:3], wref[0:3], mode)) and bits(got[3]) == bits(fused_ref.fuse(S[8:10], wref[8:10], mode))
    # a raise call whose zero-lambda vector sits in the last need only
    _, launches = counted(lambda: aspace.search_fused_batch([V[50:53], np.stack([V[53], far])], gl, TAU), asp.PanicException)
    assert launches == 0
    # no vector of any need served: B empty lists / NaN rows, nothing launched, under skip; the panic under raise
    none = [np.stack([far, far * 1.5]), far[None, :], np.stack([far * 1.5, far, far])]
    for handle in (None, sub):
        out, launches = counted(lambda: aspace.search_fused_batch(none, gl, TAU, subset=handle, on_zero_lambda="skip"))
        assert out == [[], [], []] and launches == 0
        assert counted(lambda: aspace.search_fused_batch(none, gl, TAU, subset=handle), asp.PanicException)[1] == 0
    out, launches = counted(lambda: aspace.score_fused_batch(none, gl, TAU, some, mode="max", on_zero_lambda="skip"))
    assert out.shape == (3, 257) and out.dtype == np.float64 and np.isnan(out).all() and launches == 0
    assert counted(lambda: aspace.score_fused_batch(none, gl, TAU, some), asp.PanicException)[1] == 0
    # the C entry: one status per need, lambda_q per flattened vector
    kk = min(gp["topk"], n)
    idx, sc, ln = np.zeros(6 * kk, dtype=np.int64), np.zeros(6 * kk), np.full(6, -1, dtype=np.int64)
    lq, st = np.full(14, -1.0), np.full(6, -1, dtype=np.int32)
    Vc = np.ascontiguousarray(Vf)
    rc = asp._L.as_search_fused_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 6, 14, d, TAU, None, 0, 1, None, idx.ctypes.data,
                                      sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, st.ctypes.data)
    assert rc == 0 and st.tolist() == [0, 0, asp._lib.AS_EZEROLAMBDA, 0, 0, 0] and ln.tolist() == [kk, kk, 0, kk, kk, kk]
    assert ((lq != 0.0) == np.array(want_served)).all() and (lq >= 0.0).all()
    rc = asp._L.as_search_fused_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 6, 14, d, TAU, None, 0, 0, None, idx.ctypes.data,
                                      sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, st.ctypes.data)
    Z = asp._lib.AS_EZEROLAMBDA
    assert rc == Z and st.tolist() == [0, Z, Z, 0, Z, Z] and ln.tolist() == [0] * 6


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_score_form_keeps_the_callers_order_and_duplicates(name):
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(22)
    Js = (2, 5, 1, 3)
    needs, offs = split(V[60:60 + sum(Js)], Js)
    ids = np.sort(rng.choice(n, 257, replace=False))
    S = aspace.score_items_batch(V[60:60 + sum(Js)], gl, TAU, ids)
    mixed = np.concatenate([ids[::-1][:40], ids[:3], ids[:3]])
    pos = np.searchsorted(ids, mixed)
    for mode in MODES:
        passed, wflat = need_weights(Js, 1, rng)
        got = aspace.score_fused_batch(needs, gl, TAU, mixed, weights=passed, mode=mode)
        assert got.shape == (len(Js), len(mixed)) and got.dtype == np.float64
        assert bits(got) == bits(fuse_batch(S[:, pos], offs, wflat, mode))
        # a 3-D array of equal J and a (B, J) weight array
        A = V[60:68].reshape(4, 2, -1)
        W = rng.uniform(-1.0, 1.0, (4, 2))
        S3 = aspace.score_items_batch(V[60:68], gl, TAU, ids)
        got = aspace.score_fused_batch(A, gl, TAU, mixed.tolist(), weights=W, mode=mode)
        assert bits(got) == bits(fuse_batch(S3[:, pos], [0, 2, 4, 6, 8], W.reshape(-1), mode))
    # an empty id list and an empty subset: empty answers, the lambda_q step runs
    c0 = aspace.fused_batch_counters()
    out = aspace.score_fused_batch(needs, gl, TAU, [])
    assert out.shape == (len(Js), 0) and out.dtype == np.float64
    assert aspace.search_fused_batch(needs, gl, TAU, subset=[]) == [[] for _ in Js]
    c1 = aspace.fused_batch_counters()
    assert c1["lambda_steps"] - c0["lambda_steps"] == 2 and c1["launches"] == c0["launches"]


def test_against_the_fp64_oracle(oracle_lib):
    name = "3000x96cos"
    asp, X, gp, aspace, gl, V = index(name)
    n, d = X.shape
    ref = oracle_lib.OracleIndex(X, gp)
    rng = np.random.default_rng(23)
    some = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(some)
    vecs, rows = [], []
    for q in V:   # per-vector oracle scores, as test_gpu_fused.py obtains them
        try:
            _, lq = ref.search(q, 1.0)
        except oracle_lib.ZeroLambda:
            continue
        vecs.append(q)
        rows.append(ref.scores(q, TAU, lq))
        if len(vecs) == 12:
            break
    assert len(vecs) == 12
    Js = (3, 1, 6, 2)
    needs, offs = split(np.stack(vecs), Js)
    S = np.stack(rows)
    mixed = rng.uniform(0.2, 1.0, 12) * np.where(np.arange(12) % 2 == 0, 1.0, -1.0)
    for w in (rng.uniform(0.2, 1.0, 12), mixed):
        passed = [w[offs[b]:offs[b + 1]] for b in range(len(Js))]
        for mode in MODES:
            F = fuse_batch(S, offs, w, mode)
            for ids, handle in ((np.arange(n), None), (some, sub)):
                hits = aspace.search_fused_batch(needs, gl, TAU, weights=passed, mode=mode, subset=handle)
                got = aspace.score_fused_batch(needs, gl, TAU, ids, weights=passed, mode=mode)
                for b in range(len(Js)):
                    atol = float(np.abs(passed[b]).sum()) * atol_for(d)
                    wi, ws = fused_ref.top(ids, F[b][ids], gp["topk"])
                    assert_hits_match(hits[b], list(zip(wi.tolist(), ws.tolist())), all_scores=F[b], rtol=RTOL, atol=atol)
                    np.testing.assert_allclose(got[b], F[b][ids], rtol=RTOL, atol=atol)


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_loop_of_single_calls(name):
    """The loop's lambda_q come from other `search_batch` calls: equality of bits is counted and printed, not asserted."""
    asp, X, gp, aspace, gl, V = index(name)
    n = X.shape[0]
    Js = (1, 2, 5, 8, 3, 2, 16, 4)
    needs, offs = split(V[:sum(Js)], Js)
    ids = np.arange(n)
    for mode in MODES:
        hits = aspace.search_fused_batch(needs, gl, TAU, mode=mode)
        F = aspace.score_fused_batch(needs, gl, TAU, ids, mode=mode)
        same = 0
        for b, Q in enumerate(needs):
            want = aspace.search_fused(Q, gl, TAU, mode=mode)
            wantF = aspace.score_fused(Q, gl, TAU, ids, mode=mode)
            assert_hits_match(hits[b], want, all_scores=wantF, rtol=RTOL)
            np.testing.assert_allclose(F[b], wantF, rtol=RTOL)
            same += int(hits[b] == want and bits(F[b]) == bits(wantF))
        print(f"loop comparison {name} {mode}: {same} of {len(Js)} needs agree bit for bit with the loop of single calls")


def test_errors_on_the_device_path():
    asp, X, gp, aspace, gl, V = index("1200x48")
    n, d = X.shape
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    needs = [V[:3], V[3:5]]
    sub = aspace.subset([1, 2, 3])
    wide = [np.ascontiguousarray(np.concatenate([Q, np.ones((len(Q), 1))], axis=1)) for Q in needs]
    cases = ((ValueError, "another space", lambda: other.search_fused_batch(needs, gl2, TAU, subset=sub)),
             (ValueError, "query length", lambda: aspace.search_fused_batch(wide, gl, TAU)),
             (ValueError, "query length", lambda: aspace.score_fused_batch(wide, gl, TAU, [0, 1])),
             (ValueError, "tau", lambda: aspace.search_fused_batch(needs, gl, float("nan"))),
             (ValueError, "tau", lambda: aspace.score_fused_batch(needs, gl, float("inf"), [0, 1], mode="max")),
             (ValueError, "id", lambda: aspace.score_fused_batch(needs, gl, TAU, [0, n])),
             (ValueError, "id", lambda: aspace.search_fused_batch(needs, gl, TAU, subset=[0, n])))
    for exc, match, call in cases:
        c0, o0 = aspace.fused_batch_counters(), other.fused_batch_counters()
        with pytest.raises(exc, match=match):
            call()
        assert aspace.fused_batch_counters() == c0 and other.fused_batch_counters() == o0   # nothing launched, no lambda_q step
    # the C ABI's own refusals behind the handles: a mode other than 0 / 1, a weight that is not finite
    Vc, offs = np.ascontiguousarray(np.concatenate(needs)), np.array([0, 3, 5], dtype=np.int64)
    idx, sc, ln = np.zeros(32, dtype=np.int64), np.zeros(32), np.full(2, 5, dtype=np.int64)
    for wts, mode, what in ((None, 2, "mode"), (None, -1, "mode"), (np.array([1.0, np.nan, 1.0, 1.0, 1.0]), 0, "finite"),
                            (np.array([1.0, 1.0, 1.0, 1.0, -np.inf]), 1, "finite")):
        c0 = aspace.fused_batch_counters()
        st = asp._L.as_search_fused_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU,
                                          None if wts is None else wts.ctypes.data, mode, 0, None, idx.ctypes.data, sc.ctypes.data,
                                          ln.ctypes.data, None, None)
        assert st == asp._lib.AS_EINVAL and what in asp._lib.last_error() and ln.tolist() == [0, 0]
        assert aspace.fused_batch_counters() == c0
    # the single forms and the neighbours on a handle are undisturbed by a batched call on it
    before = (aspace.search_subset(V[0], gl, TAU, sub), aspace.search_fused(V[:3], gl, TAU, subset=sub))
    aspace.search_fused_batch(needs, gl, TAU, subset=sub)
    assert (aspace.search_subset(V[0], gl, TAU, sub), aspace.search_fused(V[:3], gl, TAU, subset=sub)) == before
