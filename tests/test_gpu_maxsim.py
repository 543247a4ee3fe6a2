"""GPU: late-interaction search -- ArrowSpace.search_maxsim / score_maxsim: ONE answer to J query vectors over
groups of items, F(g) = the S13 sum over the vectors of w_j x the best score of g's members, taken and folded on the device.
Every expected value is the numpy reference tests/maxsim_ref.py over the bits `score_items_batch` returns for the same ids -- the
route there was before; labels and score bits must be equal, no tolerance (NaN is compared as NaN, not by payload).
`score_items_batch` is itself held against the fp64 oracle by tests/test_gpu_subset_batch.py.  Shapes, index and query recipe:
tests/test_gpu_fused.py's."""
import numpy as np
import pytest

import fused_ref
import maxsim_ref
from conftest import calibrate_eps, clustered

pytestmark = pytest.mark.gpu

TAU = 0.62
# (n, d, k, topk, metric, kernel): two rows of tests/test_gpu_fused.py's table
SHAPES = {"1200x48": (1200, 48, 10, 10, "l2", "gaussian"), "3000x96cos": (3000, 96, 25, 10, "cosine", "rational")}
JS = (1, 2, 8, 9, 64, 65)   # 8 / 9: the fold's rows in flight; 64 / 65: the score kernel's query tile
NVEC = 130                  # served query vectors kept per shape: three chunks of 64 under a one-MiB budget
_built = {}


def index(name):
    """One index per shape for the whole module: (asp, X, graph parameters, aspace, gl, NVEC query vectors whose lambda_q is
    not 0, their scores over every item)."""
    if name not in _built:
        import pyarrowspace_amd as asp
        n, d, k, topk, metric, kernel = SHAPES[name]
        X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
        gp = {"eps": calibrate_eps(X, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        rng = np.random.default_rng(n)
        vecs = []
        while len(vecs) < NVEC:
            q = np.ascontiguousarray(X[rng.integers(0, n)] + 0.05 * rng.standard_normal(d) / np.sqrt(d))
            if aspace.query_lambda(q, gl) != 0.0:
                vecs.append(q)
        V = np.stack(vecs)
        S = aspace.score_items_batch(V, gl, TAU, np.arange(n))
        assert not np.isnan(S).any()
        S.setflags(write=False)
        _built[name] = (asp, X, gp, aspace, gl, V, S)
    return _built[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def same_scores(got, want):
    """Equal NaN masks, equal bits elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert bits(got[ok]) == bits(want[ok])


def weights_of(J, rng):
    """(name, what the caller passes, what the reference folds with): tests/test_gpu_fused.py's."""
    rnd = rng.uniform(-1.0, 1.0, J)
    neg = np.full(J, 1.0 / J)
    neg[J // 2] = -0.75
    return [("default", None, np.full(J, 1.0 / J)), ("random", rnd, rnd), ("one negative", neg, neg)]


def label_recipes(n, rng):
    wide = np.concatenate([[-2 ** 62, -5, 2 ** 40 + 3, 2 ** 62], rng.choice(10 ** 6, 33, replace=False)])   # 37 labels, large and negative ones
    return {"groups of 10": np.arange(n) // 10, "groups of 2": np.arange(n) // 2, "1000 random": rng.integers(0, 1000, n),
            "16 random": rng.integers(0, 16, n), "one for all": np.full(n, 42), "singletons": np.arange(n),
            "wide values": wide[rng.integers(0, 37, n)]}


def without_some_groups(labels, rng):
    """Ids of a subset that leaves whole groups out: every third distinct label is dropped (a single label: half the items)."""
    u = np.unique(labels)
    if len(u) == 1:
        return np.sort(rng.choice(len(labels), len(labels) // 2, replace=False))
    return np.flatnonzero(~np.isin(labels, u[::3]))


def expected(S, labels, ids, w, served=None):
    """(labels of the groups with an item among ids, F) from the scores of every item."""
    with np.errstate(all="ignore"):
        return maxsim_ref.maxsim(S[:, ids], labels[ids], w, served)


def check_both_forms(aspace, gl, Q, grp, labels, handle, lab, F, passed, ng, rng, **kw):
    """`score_maxsim` and `search_maxsim` against (lab, F): the groups with a member and their F."""
    every = np.unique(labels)
    listed = np.concatenate([rng.permutation(every)[:300], every[:2], every[:2]])   # the caller's order, duplicates, groups left out
    want = np.full(len(listed), np.nan)
    pos = np.searchsorted(lab, listed)
    have = (pos < len(lab)) & (lab[np.minimum(pos, len(lab) - 1)] == listed)
    want[have] = F[pos[have]]
    got = aspace.score_maxsim(Q, gl, TAU, grp, listed, weights=passed, subset=handle, **kw)
    assert got.dtype == np.float64
    same_scores(got, want)
    wl, wf = maxsim_ref.top(lab, F, ng)
    hits = aspace.search_maxsim(Q, gl, TAU, grp, ng, weights=passed, subset=handle, **kw)
    assert len(hits) == min(ng, int((~np.isnan(F)).sum()))
    assert [l for l, _ in hits] == wl.tolist()
    assert bits([v for _, v in hits]) == bits(wf)
    return hits


@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_against_the_route_there_was_before(name, J):
    asp, X, gp, aspace, gl, V, S_all = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(1600 + J)
    Q, S = V[:J], S_all[:J]
    fixed = [("none", None), ("257 ids", np.sort(rng.choice(n, 257, replace=False))), ("one id", np.array([int(rng.integers(0, n))]))]
    fixed = [(sname, ids, None if ids is None else aspace.subset(ids)) for sname, ids in fixed]
    weights = weights_of(J, rng)
    turn = 0
    for lname, labels in label_recipes(n, rng).items():
        grp = aspace.groups(labels)
        part = without_some_groups(labels, rng)
        for sname, ids, handle in fixed + [("whole groups out", part, aspace.subset(part))]:
            ids = np.arange(n) if ids is None else ids
            lab, M = maxsim_ref.group_max(S[:, ids], labels[ids])
            for wname, passed, w in weights:
                F = fused_ref.fuse(M, w, "sum")
                turn += 1
                hits = check_both_forms(aspace, gl, Q, grp, labels, handle, lab, F, passed, (10, 1024, 1)[turn % 3], rng)
            if sname == "whole groups out":   # a group whose every item lies outside the subset never appears, and scores NaN
                gone = np.setdiff1d(labels, labels[ids])
                assert len(gone) == len(np.unique(labels)[::3]) or lname == "one for all"   # (one group: half of its items are out)
                assert not set(l for l, _ in hits) & set(gone.tolist())
                assert np.isnan(aspace.score_maxsim(Q, gl, TAU, grp, gone, subset=handle)).all()
        # ad-hoc labels and an ad-hoc subset give the prepared handles' answer
        want = aspace.search_maxsim(Q, gl, TAU, grp, 5, subset=fixed[1][2])
        assert aspace.search_maxsim(Q, gl, TAU, labels.tolist(), 5, subset=fixed[1][1][::-1].copy()) == want


@pytest.mark.parametrize("name", list(SHAPES))
def test_consequence_a_one_vector_names_the_heads_of_grouped_search(name):
    asp, X, gp, aspace, gl, V, S_all = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(161)
    some = np.sort(rng.choice(n, 257, replace=False))
    recipes = label_recipes(n, rng)
    for lname in ("groups of 10", "16 random", "one for all", "wide values"):   # (at most 1024 groups: every head is returned)
        grp = aspace.groups(recipes[lname])
        for handle in (None, aspace.subset(some)):
            for t in (7, 40):
                q = V[t:t + 1]
                heads = [(l, mem[0][1]) for l, mem in aspace.search_batch_grouped(q, gl, TAU, grp, 1024, 1, subset=handle)[0]]
                # S14 orders tied heads by index, S16 by label: equal wherever the scores differ
                heads.sort(key=lambda e: (-(e[1] + 0.0), e[0]))
                for ng in (1, 5, 1024):
                    got = aspace.search_maxsim(q, gl, TAU, grp, ng, weights=[1.0], subset=handle)
                    assert [l for l, _ in got] == [l for l, _ in heads[:ng]]
                    assert bits([v for _, v in got]) == bits([v + 0.0 for _, v in heads[:ng]])
                    assert aspace.search_maxsim(q, gl, TAU, grp, ng, subset=handle) == got   # the default weight of J = 1 is 1.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_consequence_b_every_item_its_own_group_is_fused_search(name):
    asp, X, gp, aspace, gl, V, S_all = index(name)
    n, topk = X.shape[0], gp["topk"]
    rng = np.random.default_rng(162)
    single = aspace.groups(np.arange(n))
    some = np.sort(rng.choice(n, 257, replace=False))
    for handle in (None, aspace.subset(some)):
        for J in (1, 3, 9):
            for wname, passed, w in weights_of(J, rng):
                fused = aspace.search_fused(V[:J], gl, TAU, weights=passed, mode="sum", subset=handle)
                for ng in (1, topk - 1, topk):
                    got = aspace.search_maxsim(V[:J], gl, TAU, single, ng, weights=passed, subset=handle)
                    assert [l for l, _ in got] == [i for i, _ in fused[:ng]]
                    assert [v for _, v in got] == [v for _, v in fused[:ng]]   # as numbers: only the sign of a zero may differ


@pytest.mark.parametrize("name", list(SHAPES))
def test_consequence_c_one_label_for_all_is_one_group(name):
    asp, X, gp, aspace, gl, V, S_all = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(163)
    one = aspace.groups(np.full(n, -9))
    some = np.sort(rng.choice(n, 257, replace=False))
    for ids, handle in ((np.arange(n), None), (some, aspace.subset(some))):
        for J in (1, 4, 9):
            for wname, passed, w in weights_of(J, rng):
                F = None
                for j in range(J):   # F = sum_j w_j max_i s_j(i), in Python floats
                    t = float(w[j]) * (float(S_all[j, ids].max()) + 0.0)
                    F = t if F is None else F + t
                got = aspace.search_maxsim(V[:J], gl, TAU, one, 3, weights=passed, subset=handle)
                assert [l for l, _ in got] == [-9] and bits([got[0][1]]) == bits([F])
                assert bits(aspace.score_maxsim(V[:J], gl, TAU, one, [-9, -9], weights=passed, subset=handle)) == bits([F, F])


@pytest.mark.parametrize("name", list(SHAPES))
def test_consequence_d_chunks_and_grid_do_not_change_the_answer(name):
    asp, X, gp, aspace, gl, V, S_all = index(name)
    n = X.shape[0]
    rng = np.random.default_rng(164)
    J = NVEC
    Q = V[:J]
    recipes = label_recipes(n, rng)
    wname, passed, w = weights_of(J, rng)[1]
    for lname in ("groups of 10", "groups of 2", "16 random"):
        labels = recipes[lname]
        grp = aspace.groups(labels)
        lab, F = expected(S_all[:J], labels, np.arange(n), w)
        c0 = aspace.maxsim_counters()
        plain = check_both_forms(aspace, gl, Q, grp, labels, None, lab, F, passed, 10, rng)
        c1 = aspace.maxsim_counters()
        # two calls under the default budget: one chunk, one pass-A launch and one fold launch each
        assert (c1["calls"] - c0["calls"], c1["vectors_served"] - c0["vectors_served"]) == (2, 2 * J)
        assert (c1["pass_a_launches"] - c0["pass_a_launches"], c1["fold_launches"] - c0["fold_launches"]) == (2, 2)
        try:
            # one MiB: 64 vectors a chunk (a vector's scores and cells take more than 8 KiB), three chunks, the last of 2 rows
            assert (1 << 20) // (8 * n + 8 * grp.ngroups) < 128
            assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
            chunked = check_both_forms(aspace, gl, Q, grp, labels, None, lab, F, passed, 10, rng)
            c2 = aspace.maxsim_counters()
            assert (c2["pass_a_launches"] - c1["pass_a_launches"], c2["fold_launches"] - c1["fold_launches"]) == (6, 6)
            assert asp._L.as_set_tuning(b"filtered_grid_cap", 2) == 0
            capped = check_both_forms(aspace, gl, Q, grp, labels, None, lab, F, passed, 10, rng)
        finally:
            assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
            assert asp._L.as_set_tuning(b"filtered_grid_cap", 0) == 0
        assert plain == chunked == capped
    # the order of positions: a subset handle lists its ids ascending whatever order they were given in
    labels = recipes["1000 random"]
    grp = aspace.groups(labels)
    some = rng.choice(n, 700, replace=False)
    assert aspace.search_maxsim(Q[:9], gl, TAU, grp, 10, subset=some) == aspace.search_maxsim(Q[:9], gl, TAU, grp, 10, subset=np.sort(some))


def test_ties_come_back_in_label_order():
    import pyarrowspace_amd as asp
    n, d = 1000, 40
    X = clustered(n, d, nclust=8, seed=6)   # tests/test_gpu_grouped.py's recipe: three identical rows
    X[500] = X[10]
    X[900] = X[10]
    gp = {"eps": calibrate_eps(X, 8), "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    q = np.ascontiguousarray(X[10] * 1.01)
    Q = np.stack([q, q])
    sb = aspace.score_items_batch(Q, gl, 1.0, np.arange(n))
    assert bits(sb[:, 10]) == bits(sb[:, 500]) == bits(sb[:, 900])   # the precondition: equal bits under both vectors
    assert (sb[:, 10] > np.delete(sb, [10, 500, 900], axis=1).max(axis=1)).all()
    for a, b, c in ((7, 3, 5), (3, 5, 7), (2 ** 40, -6, 0)):
        labels = np.arange(n) + 100
        labels[10], labels[500], labels[900] = a, b, c
        lab, F = expected(sb, labels, np.arange(n), np.array([0.25, 0.75]))
        got = aspace.search_maxsim(Q, gl, 1.0, labels, 3, weights=[0.25, 0.75])
        assert [l for l, _ in got] == sorted((a, b, c))
        assert bits([v for _, v in got]) == bits([F[np.searchsorted(lab, a)]] * 3)
        got = aspace.search_maxsim(Q, gl, 1.0, labels, 2, weights=[0.25, 0.75])   # the cut inside the tie
        assert [l for l, _ in got] == sorted((a, b, c))[:2]


def test_non_finite_items():
    """tests/test_gpu_filtered_nonfinite.py's fixture (asserted without a GPU by tests/test_filtered_nonfinite_inputs.py): an item
    with an inf scores NaN and joins no group; the all-NaN row scores its lambda term, a number."""
    import test_gpu_filtered_nonfinite as nf
    asp, fx, gp, aspace, gl, V, ref = nf.index("700x768f32")
    n = fx["X"].shape[0]
    rng = np.random.default_rng(165)
    Q = V[:5]
    S = aspace.score_items_batch(Q, gl, TAU, np.arange(n))
    assert np.isnan(S[:, fx["nan_rows"]]).all() and not np.isnan(S[:, fx["lam_rows"]]).any()
    mix = nf.subsets("700x768f32")["one-block mix"]
    for lname, labels in (("crafted", nf.grouped_labels(fx)["crafted"]), ("groups of 10", np.arange(n) // 10), ("singletons", np.arange(n))):
        grp = aspace.groups(labels)
        for ids, handle in ((np.arange(n), None), (mix, aspace.subset(mix))):
            for wname, passed, w in weights_of(5, rng):
                lab, F = expected(S, labels, ids, w)
                assert np.isnan(F).any() and not np.isnan(F).all()
                hits = check_both_forms(aspace, gl, Q, grp, labels, handle, lab, F, passed, 1024, rng)
                assert not set(l for l, _ in hits) & set(lab[np.isnan(F)].tolist())   # a group whose F is NaN is absent
        if lname == "crafted":   # group 0: the inf run alone, no member; group 1: ten numbers and ten NaN items
            got = aspace.score_maxsim(Q, gl, TAU, grp, [0, 1])
            assert np.isnan(got[0]) and not np.isnan(got[1])
    # overflowing weights: +inf, -inf and NaN out of inf - inf among the F
    tau, w = nf.OVERFLOW
    S = aspace.score_items_batch(Q[:3], gl, tau, np.arange(n))
    labels = np.arange(n) // 3
    lab, M = maxsim_ref.group_max(S, labels)
    with np.errstate(all="ignore"):
        F = fused_ref.fuse(M, w, "sum")
    assert np.isinf(F).any()
    same_scores(aspace.score_maxsim(Q[:3], gl, tau, labels, lab, weights=w), F)
    wl, wf = maxsim_ref.top(lab, F, 1024)
    got = aspace.search_maxsim(Q[:3], gl, tau, labels, 1024, weights=w)
    assert [l for l, _ in got] == wl.tolist() and bits([v for _, v in got]) == bits(wf)


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_lambda(name):
    asp, X, gp, aspace, gl, V, S_all = index(name)
    n, d = X.shape
    rng = np.random.default_rng(166)
    far = np.full(d, 50.0)   # no item within eps: lambda_q == 0 (the recipe of tests/test_gpu_fused.py)
    with pytest.raises(asp.PanicException):
        aspace.search(far, gl, TAU)
    labels = np.arange(n) // 10
    grp = aspace.groups(labels)
    ids = np.sort(rng.choice(n, 257, replace=False))
    sub = aspace.subset(ids)
    w = np.array([0.5, -0.25, 0.75, 0.4, 0.3])

    def launches():
        c = aspace.maxsim_counters()
        return c["pass_a_launches"], c["fold_launches"], c["max_atomics"]

    for at in (0, 2, 4):
        Q = V[10:15].copy()
        Q[at] = far
        served = [t != at for t in range(5)]
        for passed, wref in ((w, w), (None, np.full(5, 0.2))):
            for handle, listed in ((None, np.arange(n)), (sub, ids)):
                before = launches()
                with pytest.raises(asp.PanicException):
                    aspace.search_maxsim(Q, gl, TAU, grp, 10, weights=passed, subset=handle)
                with pytest.raises(asp.PanicException):
                    aspace.score_maxsim(Q, gl, TAU, grp, [0, 1], weights=passed, subset=handle)
                assert launches() == before   # a call that panics launches nothing of its own
                # skip: the answer over the other vectors with their own weights, not renormalised
                Sq = S_all[10:15].copy()
                Sq[at] = 123.0   # (never looked at)
                lab, F = expected(Sq, labels, listed, wref, served)
                c0 = aspace.maxsim_counters()
                check_both_forms(aspace, gl, Q, grp, labels, handle, lab, F, passed, 10, rng, on_zero_lambda="skip")
                c1 = aspace.maxsim_counters()
                assert c1["vectors_served"] - c0["vectors_served"] == 2 * 4
                # one chunk: a pass-A launch per run of served rows, one fold launch
                assert c1["pass_a_launches"] - c0["pass_a_launches"] == 2 * (2 if at == 2 else 1) and c1["fold_launches"] - c0["fold_launches"] == 2
    # a chunk whose vectors are all unserved launches nothing: vectors 64 .. 127 of 130 under a one-MiB budget
    Q = V[:NVEC].copy()
    Q[64:128] = far[None, :] * (1.0 + 0.01 * np.arange(64))[:, None]
    served = [not 64 <= t < 128 for t in range(NVEC)]
    wr = rng.uniform(-1.0, 1.0, NVEC)
    lab, F = expected(S_all[:NVEC], labels, np.arange(n), wr, served)
    try:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 1) == 0
        c0 = aspace.maxsim_counters()
        check_both_forms(aspace, gl, Q, grp, labels, None, lab, F, wr, 10, rng, on_zero_lambda="skip")
        c1 = aspace.maxsim_counters()
    finally:
        assert asp._L.as_set_tuning(b"subset_batch_mib", 256) == 0
    assert c1["fold_launches"] - c0["fold_launches"] == 2 * 2 and c1["pass_a_launches"] - c0["pass_a_launches"] == 2 * 2
    assert c1["vectors_served"] - c0["vectors_served"] == 2 * 66
    # every vector far: the panic under both settings, an empty subset included
    Qf = np.stack([far, far * 1.5, far])
    for ozl in ("raise", "skip"):
        for handle in (None, sub, []):
            before = launches()
            with pytest.raises(asp.PanicException):
                aspace.search_maxsim(Qf, gl, TAU, grp, 10, subset=handle, on_zero_lambda=ozl)
            with pytest.raises(asp.PanicException):
                aspace.score_maxsim(Qf, gl, TAU, grp, [0], subset=handle, on_zero_lambda=ozl)
            assert launches() == before


def test_no_state_survives_a_call():
    asp, X, gp, aspace, gl, V, S_all = index("3000x96cos")
    n = X.shape[0]
    rng = np.random.default_rng(167)
    every = np.arange(n)
    some = np.sort(rng.choice(n, 300, replace=False))
    sub = aspace.subset(some)
    # a large call, then small ones on the same work buffers, with other G and J, then the large one again
    plans = [(np.arange(n), 65, every, None), (np.arange(n) % 4, 2, every, None), (np.arange(n) // 2, 9, every, None),
             (np.arange(n) % 4, 1, some, sub), (np.arange(n), 3, some, sub), (np.arange(n) // 500, 64, every, None),
             (np.arange(n), 65, every, None)]
    handles = {}
    answers = []
    for labels, J, ids, handle in plans:
        grp = handles.setdefault(labels.tobytes(), aspace.groups(labels))
        w = weights_of(J, rng)[1][2]
        lab, F = expected(S_all[:J], labels, ids, w)
        answers.append(check_both_forms(aspace, gl, V[:J], grp, labels, handle, lab, F, w, 1024, rng))
    # ... and the neighbours on the handles are undisturbed
    before = aspace.search_subset(V[0], gl, TAU, sub)
    fused = aspace.search_fused(V[:3], gl, TAU)
    grouped = aspace.search_grouped(V[0], gl, TAU, np.arange(n) % 4, 3, 2)
    aspace.search_maxsim(V[:3], gl, TAU, np.arange(n) % 4, 3, subset=sub)
    aspace.search_maxsim(V[:3], gl, TAU, np.arange(n) % 4, 3)
    assert aspace.search_subset(V[0], gl, TAU, sub) == before and aspace.search_fused(V[:3], gl, TAU) == fused
    assert aspace.search_grouped(V[0], gl, TAU, np.arange(n) % 4, 3, 2) == grouped


def test_atomics_bound():
    """Section 5.17's bound: a served vector issues at most ceil(m / 64) + label changes 64-bit max-atomics over contiguous groups."""
    asp, X, gp, aspace, gl, V, S_all = index("3000x96cos")
    n = X.shape[0]
    rng = np.random.default_rng(168)
    for labels in (np.full(n, 1), np.arange(n) // 10, np.arange(n) // 2):   # (the last: more than 1024 groups, the plain form of pass A)
        changes = int((labels[1:] != labels[:-1]).sum())
        bound = -(-n // 64) + changes
        grp = aspace.groups(labels)
        for J in (1, 9):
            w = weights_of(J, rng)[1][2]
            c0 = aspace.maxsim_counters()
            got = aspace.search_maxsim(V[:J], gl, TAU, grp, 10, weights=w)
            c1 = aspace.maxsim_counters()
            lab, F = expected(S_all[:J], labels, np.arange(n), w)
            wl, wf = maxsim_ref.top(lab, F, 10)
            assert [l for l, _ in got] == wl.tolist() and bits([v for _, v in got]) == bits(wf)
            grown = c1["max_atomics"] - c0["max_atomics"]
            print(f"{grp.ngroups} groups, J = {J}: {grown} max-atomics, bound {J * bound}, {J * n} scores")
            assert 0 < grown <= J * bound
            assert (c1["calls"] - c0["calls"], c1["vectors_served"] - c0["vectors_served"]) == (1, J)
            assert (c1["pass_a_launches"] - c0["pass_a_launches"], c1["fold_launches"] - c0["fold_launches"]) == (1, 1)


def test_errors_on_the_device_path():
    asp, X, gp, aspace, gl, V, S_all = index("1200x48")
    n, d = X.shape
    other, gl2 = asp.ArrowSpaceBuilder.build(gp, X[:400].copy())
    Q = V[:3]
    grp = aspace.groups(np.arange(n) // 7)
    sub = aspace.subset([1, 2, 3])
    wide = np.ascontiguousarray(np.concatenate([Q, np.ones((3, 1))], axis=1))
    cases = ((ValueError, "another space", lambda: other.search_maxsim(Q, gl2, TAU, grp, 3)),
             (ValueError, "another space", lambda: other.score_maxsim(Q, gl2, TAU, np.arange(400), [0], subset=sub)),
             (ValueError, "query length", lambda: aspace.search_maxsim(wide, gl, TAU, grp, 3)),
             (ValueError, "query length", lambda: aspace.score_maxsim(wide, gl, TAU, grp, [0], subset=sub)),
             (ValueError, "labels", lambda: aspace.search_maxsim(Q, gl, TAU, np.arange(n - 1), 3)),
             (ValueError, "not one of the groups", lambda: aspace.score_maxsim(Q, gl, TAU, grp, [0, n])),
             (ValueError, "id", lambda: aspace.search_maxsim(Q, gl, TAU, grp, 3, subset=[0, n])))
    for exc, match, call in cases:
        c0, o0 = aspace.maxsim_counters(), other.maxsim_counters()
        with pytest.raises(exc, match=match):
            call()
        assert aspace.maxsim_counters() == c0 and other.maxsim_counters() == o0   # nothing was launched
    # the C ABI's own refusals: an unknown label, a weight that is not finite, j <= 0
    import ctypes as C
    lab, sc, ln = np.zeros(16, dtype=np.int64), np.zeros(16), C.c_int64(5)
    for j, wts, what in ((0, None, "j must be"), (3, np.array([1.0, np.nan, 1.0]), "finite")):
        st = asp._L.as_search_maxsim(aspace._h, gl._h, Q.ctypes.data, j, d, TAU, None if wts is None else wts.ctypes.data, 0, grp._h, 3, None,
                                     lab.ctypes.data, sc.ctypes.data, C.byref(ln), None, None)
        assert st == asp._lib.AS_EINVAL and what in asp._lib.last_error() and ln.value == 0
    unknown = np.array([0, 10 ** 9], dtype=np.int64)
    st = asp._L.as_score_maxsim(aspace._h, gl._h, Q.ctypes.data, 3, d, TAU, None, 0, grp._h, None, unknown.ctypes.data, 2, sc.ctypes.data, None, None)
    assert st == asp._lib.AS_EINVAL and "label 1000000000 is not one of the groups" in asp._lib.last_error()
    # an empty subset: no group has a member, but the lambda_q step runs (a far vector still panics: test_zero_lambda)
    for s in (aspace.subset([]), [], np.zeros(n, dtype=bool)):
        c0 = aspace.maxsim_counters()
        assert aspace.search_maxsim(Q, gl, TAU, grp, 3, subset=s) == []
        assert np.isnan(aspace.score_maxsim(Q, gl, TAU, grp, [0, 5, 0], subset=s)).all()
        c1 = aspace.maxsim_counters()
        assert c1["calls"] - c0["calls"] == 2 and c1["fold_launches"] == c0["fold_launches"]
    out = aspace.score_maxsim(Q, gl, TAU, grp, [])
    assert out.shape == (0,) and out.dtype == np.float64
