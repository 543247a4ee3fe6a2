"""GPU: batched late-interaction search -- ArrowSpace.search_maxsim_batch / score_maxsim_batch: B needs of J_b
query vectors each in one call, every need's group maxima folded into an accumulator row of its own on the device.  Every expected
value is the numpy reference tests/maxsim_batch_ref.py over the bits `score_items_batch` returns for the call's flattened vectors;
labels and score bits must be equal, no tolerance (NaN is compared as NaN, not by payload).  Indexes, query recipe and label
recipes: tests/test_gpu_maxsim.py's (one index per shape for the session), with more vectors drawn the same way."""
import ctypes as C

import numpy as np
import pytest

import maxsim_batch_ref as ref
from conftest import calibrate_eps, clustered
from test_gpu_maxsim import SHAPES, TAU, bits, index, same_scores, weights_of, without_some_groups

pytestmark = pytest.mark.gpu

RAGGED = (1, 2, 5, 64, 65, 3, 130, 1)   # a need cut by a chunk edge (64-row chunks), one over three chunks, J = 1 at both ends
ON_EDGES = (64, 1, 63, 128, 3)          # needs that start exactly on the edges 64, 128 and 256
NVEC = sum(RAGGED)                      # served query vectors kept per shape
_vectors = {}


def vectors(name, count=NVEC):
    """`count` query vectors of the shape whose lambda_q is not 0: test_gpu_maxsim.py's, then more by its recipe."""
    asp, X, gp, aspace, gl, V, _ = index(name)
    if name not in _vectors:
        n, d = X.shape
        rng = np.random.default_rng(7 * n + 3)
        more = []
        while V.shape[0] + len(more) < NVEC:
            q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
            if aspace.query_lambda(q, gl) != 0.0:
                more.append(q)
        _vectors[name] = np.concatenate([V, np.stack(more)])[:NVEC]
        assert _vectors[name].shape == (NVEC, d)
    assert count <= NVEC
    return _vectors[name][:count]


def scores(aspace, gl, V, ids=None, tau=TAU):
    """The reference's per-vector scores of the flattened vectors V, under whatever budgets are set: every vector served."""
    ids = np.arange(aspace.nitems) if ids is None else ids
    return aspace.score_items_batch(V, gl, tau, ids)


def split(V, Js):
    """(needs: a list of (J_b, D) arrays cut from V in order, offsets)."""
    offs = np.concatenate([[0], np.cumsum(Js)]).astype(np.int64)
    return [V[offs[b]:offs[b + 1]] for b in range(len(Js))], offs


def need_weights(Js, which, rng):
    """Per need: 0 the default, 1 random signed weights, 2 one weight of 0 -> (what the caller passes, the flattened weights
    the reference folds with)."""
    if which == 0:
        return None, ref.default_weights(np.concatenate([[0], np.cumsum(Js)]))
    per = []
    for J in Js:
        w = rng.uniform(-1.0, 1.0, J)
        if which == 2:
            w[J // 2] = 0.0
        per.append(w)
    return per, np.concatenate(per)


def label_recipes(n):
    """G = 1, an odd G, G <= 1024 contiguous, and G above the 1024 slots of pass A's combining form (interleaved labels)."""
    wide = 1100 if n < 1500 else 1500
    out = {"one for all": np.full(n, 42), "171 interleaved": np.arange(n) % 171 - 40, "groups of 10": np.arange(n) // 10,
           f"{wide} interleaved": (np.arange(n) % wide) * 3}
    assert [len(np.unique(v)) for v in out.values()] == [1, 171, n // 10, wide]
    return out


def tuning(asp, key, value):
    assert asp._L.as_set_tuning(key, value) == 0


def counted(aspace, call):
    c0 = aspace.maxsim_batch_counters()
    out = call()
    c1 = aspace.maxsim_batch_counters()
    return out, {k: c1[k] - c0[k] for k in c1}


def check_both_forms(aspace, gl, needs, offs, grp, labels, ids, handle, S, passed, wflat, ng, rng, served=None, tau=TAU, **kw):
    """`score_maxsim_batch` and `search_maxsim_batch` against the reference over S ([sum J, len(ids)], the scores of ids)."""
    with np.errstate(all="ignore"):
        lab, F = ref.maxsim_batch(S, labels[ids], offs, wflat, served)
    every = np.unique(labels)
    listed = np.concatenate([rng.permutation(every)[:300], every[:2], every[:2]])   # the caller's order, duplicates, groups left out
    want = np.full((len(needs), len(listed)), np.nan)
    pos = np.searchsorted(lab, listed)
    have = (pos < len(lab)) & (lab[np.minimum(pos, len(lab) - 1)] == listed)
    want[:, have] = F[:, pos[have]]
    got = aspace.score_maxsim_batch(needs, gl, tau, grp, listed, weights=passed, subset=handle, **kw)
    assert got.dtype == np.float64 and got.shape == want.shape
    same_scores(got, want)
    hits = aspace.search_maxsim_batch(needs, gl, tau, grp, ng, weights=passed, subset=handle, **kw)
    assert len(hits) == len(needs)
    for b, (wl, wf) in enumerate(ref.top_batch(lab, F, ng)):
        assert len(hits[b]) == min(ng, int((~np.isnan(F[b])).sum())), b
        assert [l for l, _ in hits[b]] == wl.tolist(), b
        assert bits([v for _, v in hits[b]]) == bits(wf), b
    return got, hits


@pytest.mark.parametrize("Js", [RAGGED, ON_EDGES], ids=["ragged", "on edges"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_ragged_needs_across_chunk_edges(name, Js):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(1700 + len(Js))
    V = vectors(name, sum(Js))
    needs, offs = split(V, Js)
    S_all = scores(aspace, gl, V)   # the reference's scores, under the default budget
    assert not np.isnan(S_all).any()   # every vector is served
    half = np.sort(rng.choice(n, n // 2, replace=False))
    turn = 0
    for lname, labels in label_recipes(n).items():
        grp = aspace.groups(labels)
        part = without_some_groups(labels, rng)
        for sname, ids in (("none", None), ("a random half", half), ("whole groups out", part)):
            handle = None if ids is None else aspace.subset(ids)
            ids = np.arange(n) if ids is None else ids
            S = S_all[:, ids]
            try:
                tuning(asp, b"subset_batch_mib", 1)   # 64 vectors a chunk: a vector's scores and cells take more than 8 KiB
                assert (1 << 20) // (8 * len(ids) + 8 * grp.ngroups) < 128 or sname != "none"
                for which in range(3):
                    passed, wflat = need_weights(Js, which, rng)
                    turn += 1
                    _, d = counted(aspace, lambda: check_both_forms(aspace, gl, needs, offs, grp, labels, ids, handle, S, passed, wflat,
                                                                    (10, 1024, 1)[turn % 3], rng))
                    assert (d["calls"], d["needs"], d["lambda_steps"], d["need_groups"]) == (2, 2 * len(Js), 2, 2)
                    assert d["vectors_served"] == 2 * sum(Js) and d["fold_launches"] > 2   # the chunking happened
                    if sname == "none":   # 64 rows a chunk: ceil(sum J / 64) fold launches a call, one pass-A launch a chunk
                        assert d["fold_launches"] == d["pass_a_launches"] == 2 * -(-sum(Js) // 64)
            finally:
                tuning(asp, b"subset_batch_mib", 256)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_answer_does_not_depend_on_the_need_groups(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(171)
    Js = RAGGED
    V = vectors(name, sum(Js))
    needs, offs = split(V, Js)
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    some = np.sort(rng.choice(n, 257, replace=False))
    S_all = scores(aspace, gl, V)
    row = 8 * grp.ngroups   # bytes of an accumulator row
    # KiB budgets (negative values) that hold exactly one and exactly two rows; the default holds every need
    one, two = -(-row // 1024), -(-2 * row // 1024)
    assert row <= one * 1024 < 2 * row and 2 * row <= two * 1024 < 3 * row
    for ids, handle in ((np.arange(n), None), (some, aspace.subset(some))):
        seen = []
        try:
            for setting, groups in ((-one, len(Js)), (-two, -(-len(Js) // 2)), (0, 1)):
                tuning(asp, b"maxsim_batch_mib", setting)
                passed, wflat = need_weights(Js, 1, np.random.default_rng(172))
                (got, hits), d = counted(aspace, lambda: check_both_forms(aspace, gl, needs, offs, grp, labels, ids, handle, S_all[:, ids],
                                                                          passed, wflat, 10, np.random.default_rng(173)))
                assert d["need_groups"] == 2 * groups and d["lambda_steps"] == 2
                seen.append((bits(got[~np.isnan(got)]), hits))
        finally:
            tuning(asp, b"maxsim_batch_mib", 0)
        assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("name", list(SHAPES))
def test_later_loop_trips_return_the_same_bits(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    Js = (3, 1, 9, 2)
    V = vectors(name, sum(Js))
    needs, offs = split(V, Js)
    S_all = scores(aspace, gl, V)
    # 599 groups: an odd G whose single last group falls into the second trip of the fold under a cap of 1 (256 pairs a trip);
    # n // 2 groups: three trips at the larger shape; 171: one trip
    for labels in (np.minimum(np.arange(n) // 2, 598), np.arange(n) // 2, np.arange(n) % 171):
        grp = aspace.groups(labels)
        passed, wflat = need_weights(Js, 1, np.random.default_rng(174))
        args = (aspace, gl, needs, offs, grp, labels, np.arange(n), None, S_all, passed, wflat, 1024)
        want = check_both_forms(*args, np.random.default_rng(175))
        try:
            for cap in (1, 3):
                tuning(asp, b"filtered_grid_cap", cap)
                got = check_both_forms(*args, np.random.default_rng(175))
                same_scores(got[0], want[0])
                assert got[1] == want[1]
        finally:
            tuning(asp, b"filtered_grid_cap", 0)


@pytest.mark.parametrize("J", [1, 9, 65])
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_need_is_the_single_form_bit_for_bit(name, J):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(176 + J)
    Q = vectors(name)[20:20 + J]
    some = np.sort(rng.choice(n, 257, replace=False))
    for lname, labels in label_recipes(n).items():
        grp = aspace.groups(labels)
        listed = np.concatenate([rng.permutation(np.unique(labels))[:50], labels[:2]])
        for handle in (None, aspace.subset(some)):
            for wname, passed, w in weights_of(J, rng):
                want = aspace.search_maxsim(Q, gl, TAU, grp, 10, weights=passed, subset=handle)
                got = aspace.search_maxsim_batch(Q[None], gl, TAU, grp, 10, weights=None if passed is None else [passed], subset=handle)
                assert len(got) == 1 and [l for l, _ in got[0]] == [l for l, _ in want]
                assert bits([v for _, v in got[0]]) == bits([v for _, v in want])
                wantF = aspace.score_maxsim(Q, gl, TAU, grp, listed, weights=passed, subset=handle)
                gotF = aspace.score_maxsim_batch([Q], gl, TAU, grp, listed, weights=None if passed is None else passed[None], subset=handle)
                assert gotF.shape == (1, len(listed))
                same_scores(gotF[0], wantF)


@pytest.mark.parametrize("name", list(SHAPES))
def test_needs_of_one_vector_name_the_heads_of_grouped_search(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(177)
    Q = vectors(name)[5:16]   # 11 needs of one vector each
    some = np.sort(rng.choice(n, 257, replace=False))
    for lname in ("one for all", "171 interleaved", "groups of 10"):   # (at most 1024 groups: every head is returned)
        grp = aspace.groups(label_recipes(n)[lname])
        for handle in (None, aspace.subset(some)):
            grouped = aspace.search_batch_grouped(Q, gl, TAU, grp, 1024, 1, subset=handle)
            for ng in (1, 5, 1024):
                got = aspace.search_maxsim_batch(Q[:, None, :], gl, TAU, grp, ng, weights=np.ones((len(Q), 1)), subset=handle)
                assert got == aspace.search_maxsim_batch(Q[:, None, :], gl, TAU, grp, ng, subset=handle)   # the default weight of J = 1 is 1.0
                for b in range(len(Q)):
                    heads = [(l, mem[0][1]) for l, mem in grouped[b]]
                    # S14 orders tied heads by index, S17 by label: equal wherever the scores differ
                    heads.sort(key=lambda e: (-(e[1] + 0.0), e[0]))
                    assert [l for l, _ in got[b]] == [l for l, _ in heads[:ng]]
                    assert bits([v for _, v in got[b]]) == bits([v + 0.0 for _, v in heads[:ng]])


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_item_its_own_group_is_batched_fused_search(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n, topk = X.shape[0], gp["topk"]
    rng = np.random.default_rng(178)
    Js = (1, 3, 9, 2)
    needs, offs = split(vectors(name, sum(Js)), Js)
    single = aspace.groups(np.arange(n))
    some = np.sort(rng.choice(n, 257, replace=False))
    for handle in (None, aspace.subset(some)):
        for which in range(3):
            passed, wflat = need_weights(Js, which, rng)
            fused = aspace.search_fused_batch(needs, gl, TAU, weights=passed, mode="sum", subset=handle)
            for ng in (1, topk):
                got = aspace.search_maxsim_batch(needs, gl, TAU, single, ng, weights=passed, subset=handle)
                for b in range(len(Js)):
                    assert [l for l, _ in got[b]] == [i for i, _ in fused[b][:ng]]
                    assert bits([v for _, v in got[b]]) == bits([v for _, v in fused[b][:ng]])


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


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_lambda(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n, d = X.shape
    V = vectors(name)
    rng = np.random.default_rng(179)
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0 (the recipe of tests/test_gpu_maxsim.py::test_zero_lambda)
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, TAU)
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    some = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(some)
    # such a vector first, in the middle and last in a need; a need made only of such vectors between ordinary needs
    needs = [V[50:53], np.stack([far, V[53], V[54]]), np.stack([V[55], far * 1.5, V[56]]), np.stack([far, far * 1.5]), V[57:59],
             np.stack([V[59], V[60], far])]
    Vf, offs = np.concatenate(needs), np.array([0, 3, 6, 9, 11, 13, 16])
    want_served = [True] * 3 + [False, True, True] + [True, False, True] + [False, False] + [True, True] + [True, True, False]
    weights = [None, [0.5, -0.25, 0.75], [0.4, 0.3, -0.2], None, [2.0, 1.0], None]
    wflat = np.array([1.0 / 3] * 3 + [0.5, -0.25, 0.75] + [0.4, 0.3, -0.2] + [0.5, 0.5] + [2.0, 1.0] + [1.0 / 3] * 3)
    moved = ("vectors_served", "pass_a_launches", "max_atomics", "fold_launches", "need_groups")

    for ids, handle in ((np.arange(n), None), (some, sub)):
        S, served = per_vector_scores(asp, aspace, gl, Vf, ids)
        assert served == want_served
        for passed, wref in ((weights, wflat), (None, ref.default_weights(offs))):
            # raise: the panic of the whole call with nothing gathered: the counters do not move past the lambda_q step
            for call in (lambda: aspace.search_maxsim_batch(needs, gl, TAU, grp, 10, weights=passed, subset=handle),
                         lambda: aspace.score_maxsim_batch(needs, gl, TAU, grp, [0, 1], weights=passed, subset=handle)):
                c0 = aspace.maxsim_batch_counters()
                with pytest.raises(asp.PanicException):
                    call()
                c1 = aspace.maxsim_batch_counters()
                assert (c1["calls"] - c0["calls"], c1["needs"] - c0["needs"], c1["lambda_steps"] - c0["lambda_steps"]) == (1, 6, 1)
                assert all(c1[k] == c0[k] for k in moved)
            # skip: the served vectors of each need with their own weights, not renormalised; need 3 has none left
            (got, hits), dc = counted(aspace, lambda: check_both_forms(aspace, gl, needs, offs, grp, labels, ids, handle, S, passed, wref, 10,
                                                                       rng, served=served, on_zero_lambda="skip"))
            assert hits[3] == [] and np.isnan(got[3]).all() and not np.isnan(got[[0, 1, 2, 4, 5]]).all(axis=1).any()
            assert dc["vectors_served"] == 2 * 11 and dc["fold_launches"] == 2
            assert dc["pass_a_launches"] == 2 * 4   # one chunk: a pass-A launch per run of served rows (0 .. 2, 4 .. 6, 8, 11 .. 14)
    # a need made only of such vectors that sits at a chunk edge (rows 64 .. 127 of 64-row chunks), a cut need on either side
    Js = (60, 4, 64, 2, 1)
    Q = V[:sum(Js)].copy()
    Q[64:128] = far[None, :] * (1.0 + 0.01 * np.arange(64))[:, None]
    Q[60] = far
    Q[130] = far * 2.0
    needs, offs = split(Q, Js)
    S, served = per_vector_scores(asp, aspace, gl, Q, np.arange(n))
    assert served == [not (64 <= t < 128 or t in (60, 130)) for t in range(sum(Js))]
    passed, wflat = need_weights(Js, 1, rng)
    try:
        tuning(asp, b"subset_batch_mib", 1)
        (got, hits), dc = counted(aspace, lambda: check_both_forms(aspace, gl, needs, offs, grp, labels, np.arange(n), None, S, passed, wflat,
                                                                   10, rng, served=served, on_zero_lambda="skip"))
    finally:
        tuning(asp, b"subset_batch_mib", 256)
    assert hits[2] == [] and np.isnan(got[2]).all() and hits[4] == [] and np.isnan(got[4]).all()
    # the chunk of rows 64 .. 127 launches nothing; chunk 0: rows 0 .. 59 and 61 .. 63; chunk 2: row 128, row 129
    assert dc["fold_launches"] == 2 * 2 and dc["pass_a_launches"] == 2 * 3 and dc["vectors_served"] == 2 * 65
    # no vector of any need served: B empty lists / NaN rows under skip, nothing launched; the panic under raise
    none = [np.stack([far, far * 1.5]), far[None, :], np.stack([far * 1.5, far, far])]
    for handle in (None, sub, []):
        out, dc = counted(aspace, lambda: aspace.search_maxsim_batch(none, gl, TAU, grp, 3, subset=handle, on_zero_lambda="skip"))
        assert out == [[], [], []] and all(dc[k] == 0 for k in moved) and dc["lambda_steps"] == 1
        out, dc = counted(aspace, lambda: aspace.score_maxsim_batch(none, gl, TAU, grp, [0, 5, 0], subset=handle, on_zero_lambda="skip"))
        assert out.shape == (3, 3) and np.isnan(out).all() and all(dc[k] == 0 for k in moved)
        with pytest.raises(asp.PanicException):
            aspace.search_maxsim_batch(none, gl, TAU, grp, 3, subset=handle)
    # the C entry: one status per need, lambda_q per flattened vector
    needs = [V[50:53], np.stack([far, V[53]]), np.stack([far, far * 1.5]), V[57:59]]
    Vc, offs = np.ascontiguousarray(np.concatenate(needs)), np.array([0, 3, 5, 7, 9], dtype=np.int64)
    lab, sc, ln = np.zeros(4 * 10, dtype=np.int64), np.zeros(4 * 10), np.full(4, -1, dtype=np.int64)
    lq, st = np.full(9, -1.0), np.full(4, -1, dtype=np.int32)
    Z = asp._lib.AS_EZEROLAMBDA
    for skip, rc_want, st_want, ln_want in ((1, 0, [0, 0, Z, 0], [10, 10, 0, 10]), (0, Z, [0, Z, Z, 0], [0, 0, 0, 0])):
        rc = asp._L.as_search_maxsim_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 4, 9, d, TAU, None, skip, grp._h, 10, None,
                                           lab.ctypes.data, sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, st.ctypes.data)
        assert rc == rc_want and st.tolist() == st_want and ln.tolist() == ln_want
        assert ((lq != 0.0) == np.array([True] * 3 + [False, True] + [False, False] + [True, True])).all() and (lq >= 0.0).all()


def test_ties_come_back_in_label_order_per_need():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)   # tests/test_gpu_maxsim.py's recipe: three identical rows
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q, r = np.ascontiguousarray(X[10] * 1.01), np.ascontiguousarray(X[10] * 0.99)
    needs = [np.stack([q, r]), q[None, :], np.stack([r, q, r])]
    Vf, offs = np.concatenate(needs), np.array([0, 2, 3, 6])
    weights = [[0.25, 0.75], None, [0.5, 0.25, 0.125]]
    wflat = np.array([0.25, 0.75, 1.0, 0.5, 0.25, 0.125])
    sb = aspace.score_items_batch(Vf, gl, 1.0, np.arange(n))
    assert bits(sb[:, 10]) == bits(sb[:, 500]) == bits(sb[:, 900])   # the precondition: equal bits under every vector
    assert (sb[:, 10] > np.delete(sb, [10, 500, 900], axis=1).max(axis=1)).all()
    for a, b, c in ((7, 3, 5), (3, 5, 7), (2 ** 40, -6, 0)):
        labels = np.arange(n) + 100
        labels[10], labels[500], labels[900] = a, b, c
        lab, F = ref.maxsim_batch(sb, labels, offs, wflat)
        for ng in (3, 2):   # the whole tie; the cut inside the tie
            got = aspace.search_maxsim_batch(needs, gl, 1.0, labels, ng, weights=weights)
            for y in range(3):
                assert [l for l, _ in got[y]] == sorted((a, b, c))[:ng]
                assert bits([v for _, v in got[y]]) == bits([F[y, np.searchsorted(lab, a)]] * ng)


def test_non_finite_items_and_a_need_that_cancels():
    """tests/test_gpu_filtered_nonfinite.py's fixture: an item with an inf scores NaN and is no member; a group of such items
    alone is absent from the search form and NaN in the score form; a +1 / -1 need cancels to +0.0 between two ordinary needs."""
    import test_gpu_filtered_nonfinite as nf
    asp, fx, gp, aspace, gl, V, _ = nf.index("700x768f32")
    n = fx["X"].shape[0]
    rng = np.random.default_rng(180)
    needs = [V[:3], np.stack([V[3], V[3]]), V[3:5]]
    Vf, offs = np.concatenate(needs), np.array([0, 3, 5, 7])
    weights = [None, [1.0, -1.0], [0.25, -2.0]]
    wflat = np.array([1.0 / 3] * 3 + [1.0, -1.0] + [0.25, -2.0])
    S = aspace.score_items_batch(Vf, gl, TAU, np.arange(n))
    assert np.isnan(S[:, fx["nan_rows"]]).all() and not np.isnan(S[:, fx["lam_rows"]]).any()
    mix = nf.subsets("700x768f32")["one-block mix"]
    for lname, labels in (("crafted", nf.grouped_labels(fx)["crafted"]), ("groups of 10", np.arange(n) // 10), ("singletons", np.arange(n))):
        grp = aspace.groups(labels)
        for ids, handle in ((np.arange(n), None), (mix, aspace.subset(mix))):
            with np.errstate(all="ignore"):
                lab, F = ref.maxsim_batch(S[:, ids], labels[ids], offs, wflat)
            assert np.isnan(F).any(axis=1).all() and not np.isnan(F).all(axis=1).any()
            got, hits = check_both_forms(aspace, gl, needs, offs, grp, labels, ids, handle, S[:, ids], weights, wflat, 1024, rng)
            for y in range(3):
                assert not set(l for l, _ in hits[y]) & set(lab[np.isnan(F[y])].tolist())   # a group whose F is NaN is absent
            # the +1 / -1 need: +0.0 for every group with a member, in label order
            alive = lab[~np.isnan(F[1])]
            assert bits(F[1][~np.isnan(F[1])]) == bits(np.zeros(len(alive)))
            assert [l for l, _ in hits[1]] == alive[:1024].tolist() and bits([v for _, v in hits[1]]) == bits(np.zeros(min(len(alive), 1024)))
            assert np.nanmax(np.abs(F[0])) > 0.0 and np.nanmax(np.abs(F[2])) > 0.0
        if lname == "crafted":   # group 0: the inf run alone, no member; group 1: ten numbers and ten NaN items
            got = aspace.score_maxsim_batch(needs, gl, TAU, grp, [0, 1], weights=weights)
            assert np.isnan(got[:, 0]).all() and not np.isnan(got[:, 1]).any()


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_score_form_keeps_the_callers_order_and_duplicates(name):
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(181)
    Js = (2, 5, 1, 3)
    Vf = vectors(name)[60:60 + sum(Js)]
    needs, offs = split(Vf, Js)
    labels = np.arange(n) // 10 * 7 - 50
    grp = aspace.groups(labels)
    S = scores(aspace, gl, Vf)
    passed, wflat = need_weights(Js, 1, rng)
    lab, F = ref.maxsim_batch(S, labels, offs, wflat)
    mixed = np.concatenate([lab[::-1][:40], lab[:3], lab[:3]])
    got = aspace.score_maxsim_batch(needs, gl, TAU, grp, mixed, weights=passed)
    assert got.shape == (len(Js), len(mixed)) and got.dtype == np.float64
    assert bits(got) == bits(F[:, np.searchsorted(lab, mixed)])
    # a 3-D array of equal J, a (B, J) weight array, ad-hoc labels and a list of labels
    A = Vf[:8].reshape(4, 2, -1)
    W = rng.uniform(-1.0, 1.0, (4, 2))
    lab3, F3 = ref.maxsim_batch(scores(aspace, gl, Vf[:8]), labels, [0, 2, 4, 6, 8], W.reshape(-1))
    got = aspace.score_maxsim_batch(A, gl, TAU, labels.tolist(), mixed.tolist(), weights=W)
    assert bits(got) == bits(F3[:, np.searchsorted(lab3, mixed)])
    # no label listed, and an empty subset: empty answers / NaN, the lambda_q step runs, nothing is folded
    (out, hits, nan), dc = counted(aspace, lambda: (aspace.score_maxsim_batch(needs, gl, TAU, grp, []),
                                                    aspace.search_maxsim_batch(needs, gl, TAU, grp, 3, subset=[]),
                                                    aspace.score_maxsim_batch(needs, gl, TAU, grp, [-50, -43, -50], subset=[])))
    assert out.shape == (len(Js), 0) and out.dtype == np.float64
    assert hits == [[] for _ in Js] and nan.shape == (len(Js), 3) and np.isnan(nan).all()
    assert dc["lambda_steps"] == 3 and dc["calls"] == 3 and dc["fold_launches"] == 0 and dc["need_groups"] == 0


def test_no_state_survives_a_call():
    asp, X, gp, aspace, gl, _, _ = index("3000x96cos")
    n = X.shape[0]
    V = vectors("3000x96cos")
    rng = np.random.default_rng(182)
    every = np.arange(n)
    some = np.sort(rng.choice(n, 300, replace=False))
    sub = aspace.subset(some)
    # a large call, then small ones on the same work buffers, with other G, B and J, then the large one again
    plans = [(np.arange(n), (65, 3), every, None), (np.arange(n) % 4, (2,), every, None), (np.arange(n) // 2, (9, 1, 1), every, None),
             (np.arange(n) % 4, (1, 1, 1, 1, 1), some, sub), (np.arange(n), (3, 2), some, sub), (np.arange(n) // 500, (64, 1), every, None),
             (np.arange(n), (65, 3), every, None)]
    handles = {}
    for labels, Js, ids, handle in plans:
        grp = handles.setdefault(labels.tobytes(), aspace.groups(labels))
        Vf = V[:sum(Js)]
        needs, offs = split(Vf, Js)
        passed, wflat = need_weights(Js, 1, rng)
        check_both_forms(aspace, gl, needs, offs, grp, labels, ids, handle, scores(aspace, gl, Vf, ids), passed, wflat, 1024, rng)
    # the single forms and the batched forms alternate on one handle: neither disturbs the other, nor the neighbours
    labels = np.arange(n) % 7
    grp = aspace.groups(labels)
    needs = [V[:3], V[3:12]]
    listed = [0, 3, 6]
    for handle in (None, sub):
        single = (aspace.search_maxsim(V[:9], gl, TAU, grp, 5, subset=handle), bits(aspace.score_maxsim(V[:9], gl, TAU, grp, listed, subset=handle)))
        batch = (aspace.search_maxsim_batch(needs, gl, TAU, grp, 5, subset=handle),
                 bits(aspace.score_maxsim_batch(needs, gl, TAU, grp, listed, subset=handle)))
        others = (aspace.search_fused(V[:3], gl, TAU, subset=handle), aspace.search_grouped(V[0], gl, TAU, grp, 3, 2, subset=handle),
                  aspace.search_fused_batch(needs, gl, TAU, subset=handle))
        for _ in range(2):
            assert aspace.search_maxsim(V[:9], gl, TAU, grp, 5, subset=handle) == single[0]
            assert aspace.search_maxsim_batch(needs, gl, TAU, grp, 5, subset=handle) == batch[0]
            assert bits(aspace.score_maxsim(V[:9], gl, TAU, grp, listed, subset=handle)) == single[1]
            assert bits(aspace.score_maxsim_batch(needs, gl, TAU, grp, listed, subset=handle)) == batch[1]
        assert (aspace.search_fused(V[:3], gl, TAU, subset=handle), aspace.search_grouped(V[0], gl, TAU, grp, 3, 2, subset=handle),
                aspace.search_fused_batch(needs, gl, TAU, subset=handle)) == others


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_loop_of_single_calls(name):
    """The loop's lambda_q come from other `search_batch` calls: every need must agree with the numpy reference over the call's
    own vectors; agreement with the loop of `search_maxsim` / `score_maxsim` calls is counted and printed, not asserted."""
    asp, X, gp, aspace, gl, _, _ = index(name)
    n = X.shape[0]
    Js = (1, 2, 5, 8, 3, 2, 16, 4)
    Vf = vectors(name, sum(Js))
    needs, offs = split(Vf, Js)
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    every = np.unique(labels)
    got, hits = check_both_forms(aspace, gl, needs, offs, grp, labels, np.arange(n), None, scores(aspace, gl, Vf), None,
                                 ref.default_weights(offs), 10, np.random.default_rng(183))
    F = aspace.score_maxsim_batch(needs, gl, TAU, grp, every)
    same = 0
    for b, Q in enumerate(needs):
        same += int(hits[b] == aspace.search_maxsim(Q, gl, TAU, grp, 10) and bits(F[b]) == bits(aspace.score_maxsim(Q, gl, TAU, grp, every)))
    print(f"loop comparison {name}: {same} of {len(Js)} needs agree bit for bit with the loop of single calls")


def test_errors_on_the_device_path():
    asp, X, gp, aspace, gl, _, _ = index("1200x48")
    n, d = X.shape
    V = vectors("1200x48")
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    needs = [V[:3], V[3:5]]
    grp = aspace.groups(np.arange(n) // 7)
    sub = aspace.subset([1, 2, 3])
    wide = [np.ascontiguousarray(np.concatenate([Q, np.ones((len(Q), 1))], axis=1)) for Q in needs]
    cases = ((ValueError, "another space", lambda: other.search_maxsim_batch(needs, gl2, TAU, grp, 3)),
             (ValueError, "another space", lambda: other.score_maxsim_batch(needs, gl2, TAU, np.arange(400), [0], subset=sub)),
             (ValueError, "query length", lambda: aspace.search_maxsim_batch(wide, gl, TAU, grp, 3)),
             (ValueError, "query length", lambda: aspace.score_maxsim_batch(wide, gl, TAU, grp, [0], subset=sub)),
             (ValueError, "labels", lambda: aspace.search_maxsim_batch(needs, gl, TAU, np.arange(n - 1), 3)),
             (ValueError, "not one of the groups", lambda: aspace.score_maxsim_batch(needs, gl, TAU, grp, [0, n])),
             (ValueError, "id", lambda: aspace.search_maxsim_batch(needs, gl, TAU, grp, 3, subset=[0, n])))
    for exc, match, call in cases:
        c0, o0 = aspace.maxsim_batch_counters(), other.maxsim_batch_counters()
        with pytest.raises(exc, match=match):
            call()
        assert aspace.maxsim_batch_counters() == c0 and other.maxsim_batch_counters() == o0   # nothing launched, no lambda_q step
    # the C ABI's own refusals behind the handles: a wrong d, a weight that is not finite, an unknown label -- AS_EINVAL, the
    # lengths reset, nothing else written
    Vc, offs = np.ascontiguousarray(np.concatenate(needs)), np.array([0, 3, 5], dtype=np.int64)
    lab, sc, ln = np.full(6, 7, dtype=np.int64), np.full(6, 5.0), np.full(2, 9, dtype=np.int64)
    lq, st = np.full(5, 3.0), np.full(2, 9, dtype=np.int32)
    for dd, wts, what in ((d + 1, None, "query length"), (d - 1, None, "query length"), (d, np.array([1.0, np.nan, 1.0, 1.0, 1.0]), "finite")):
        ln[:] = 9
        c0 = aspace.maxsim_batch_counters()
        rc = asp._L.as_search_maxsim_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, dd, TAU,
                                           None if wts is None else wts.ctypes.data, 0, grp._h, 3, None, lab.ctypes.data, sc.ctypes.data,
                                           ln.ctypes.data, lq.ctypes.data, st.ctypes.data)
        assert rc == asp._lib.AS_EINVAL and what in asp._lib.last_error() and ln.tolist() == [0, 0]
        assert lab.tolist() == [7] * 6 and sc.tolist() == [5.0] * 6 and lq.tolist() == [3.0] * 5 and st.tolist() == [9, 9]
        rc = asp._L.as_score_maxsim_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, dd, TAU,
                                          None if wts is None else wts.ctypes.data, 0, grp._h, None, lab.ctypes.data, 2, sc.ctypes.data,
                                          lq.ctypes.data, st.ctypes.data)
        assert rc == asp._lib.AS_EINVAL and what in asp._lib.last_error()
        assert sc.tolist() == [5.0] * 6 and lq.tolist() == [3.0] * 5 and st.tolist() == [9, 9]
        assert aspace.maxsim_batch_counters() == c0
    unknown = np.array([0, 10 ** 9], dtype=np.int64)
    rc = asp._L.as_score_maxsim_batch(aspace._h, gl._h, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp._h, None,
                                      unknown.ctypes.data, 2, sc.ctypes.data, None, None)
    assert rc == asp._lib.AS_EINVAL and "label 1000000000 is not one of the groups" in asp._lib.last_error() and sc.tolist() == [5.0] * 6


def test_a_shard_of_a_row_sharded_index_is_not_supported():
    """A 200-row shard at row offset 200 of 600 items (tests/test_gpu_shardgraph.py's way to make one): AS_EUNSUPPORTED from
    both entries, nothing written but the lengths."""
    import torch

    import pyarrowspace_amd as asp
    from pyarrowspace_amd.dist import HipEngine
    n, d, k, lo, hi = 600, 32, 5, 200, 400
    X = clustered(n, d, nclust=4, seed=9)
    gp = {"eps": calibrate_eps(X, k), "k": k, "topk": 5, "p": 2.0, "sigma": None}
    whole = HipEngine(gp)
    whole.create_space(torch.from_numpy(X).cuda())
    idx, dist, gy, cnt = whole.knn_rows(0, n)
    valid = torch.arange(k, device=idx.device)[None, :] < cnt[:, None].long()
    src = torch.arange(n, device=idx.device)[:, None].expand(n, k)[valid]
    tgt, ed, eg = idx[valid].long(), dist[valid], gy[valid]
    here = (tgt >= lo) & (tgt < hi)
    e = HipEngine(gp)
    e.create_space(torch.from_numpy(X[lo:hi].copy()).cuda())
    e.graph_shard_csr(n, lo, idx[lo:hi].contiguous(), dist[lo:hi].contiguous(), gy[lo:hi].contiguous(), cnt[lo:hi].contiguous(),
                      (tgt[here] - lo).int(), src[here].int(), ed[here], eg[here])
    assert int(e.L.as_graph_row_offset(e.gr)) == lo and int(e.L.as_graph_ncols(e.gr)) == n
    labels = np.ascontiguousarray(np.arange(hi - lo) // 10, dtype=np.int64)
    grp = C.c_void_p()
    assert e.L.as_groups_create(e.sp, labels.ctypes.data, hi - lo, C.byref(grp)) == 0
    Vc, offs = np.ascontiguousarray(X[lo:lo + 5]), np.array([0, 3, 5], dtype=np.int64)
    lab, sc, ln = np.full(6, 7, dtype=np.int64), np.full(6, 5.0), np.full(2, 9, dtype=np.int64)
    lq, st = np.full(5, 3.0), np.full(2, 9, dtype=np.int32)
    try:
        rc = e.L.as_search_maxsim_batch(e.sp, e.gr, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp, 3, None, lab.ctypes.data,
                                        sc.ctypes.data, ln.ctypes.data, lq.ctypes.data, st.ctypes.data)
        assert rc == asp._lib.AS_EUNSUPPORTED and "row-sharded" in asp._lib.last_error() and ln.tolist() == [0, 0]
        rc = e.L.as_score_maxsim_batch(e.sp, e.gr, Vc.ctypes.data, offs.ctypes.data, 2, 5, d, TAU, None, 0, grp, None, lab.ctypes.data, 2,
                                       sc.ctypes.data, lq.ctypes.data, st.ctypes.data)
        assert rc == asp._lib.AS_EUNSUPPORTED and "row-sharded" in asp._lib.last_error()
        assert lab.tolist() == [7] * 6 and sc.tolist() == [5.0] * 6 and lq.tolist() == [3.0] * 5 and st.tolist() == [9, 9]
        out = (C.c_int64 * 8)()
        assert e.L.as_maxsim_batch_counters(e.sp, out, 8) == 0 and list(out) == [0] * 8
    finally:
        e.L.as_groups_free(grp)
        e.close()
        whole.close()
