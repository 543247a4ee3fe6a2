"""CPU: the poisoned fixtures of tests/test_gpu_filtered_nonfinite.py are what that file takes them for.  Through the fp64
oracle and the numpy references: a row with an inf anywhere scores NaN at every tau and for every query, a row whose norm is NaN
or zero scores its lambda term (+0.0 at tau = 1), every poisoned row has lambda 0 and every lambda is finite, an overflow row is
NaN for its own query alone, the references order NaN as DESIGN.md section 2 says, and each crafted case holds what its name
promises."""
import numpy as np
import pytest

import diverse_ref
import fused_ref
import grouped_ref
import test_gpu_filtered_nonfinite as nf

_ref = {}


def test_the_grid_cap_is_a_tuning_key():
    import os
    import pyarrowspace_amd as asp
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arrowspace_hip.h")).read()
    assert '"filtered_grid_cap"' in hdr
    try:
        assert asp._L.as_set_tuning(b"filtered_grid_cap", 2) == 0
    finally:
        assert asp._L.as_set_tuning(b"filtered_grid_cap", 0) == 0
    assert asp._L.as_set_tuning(b"filtered_grid_caps", 2) == 1   # an unknown key


def oracle(name, oracle_lib):
    if name not in _ref:
        fx = nf.poisoned(name)
        ref = oracle_lib.OracleIndex(fx["X"], fx["gp"])
        V = nf.queries(name, lambda q: ref.query_lambda(q) != 0.0)
        _ref[name] = (fx, ref, V, np.array([ref.query_lambda(q) for q in V]))
    return _ref[name]


@pytest.mark.parametrize("name", nf.NAMES)
def test_the_poison_is_where_the_fixture_says(name):
    fx = nf.poisoned(name)
    X, clean, rows = fx["X"], fx["clean"], fx["rows"]
    n, d, k, topk, metric, kernel, f32, (r0, r1), with_huge = nf.SHAPES[name]
    assert np.isfinite(clean).all() and np.array_equal(np.delete(X, fx["bad"], axis=0), np.delete(clean, fx["bad"], axis=0))
    assert ((X[rows["pinf"] + rows["run"] + rows["inf_at_zcol"]] == np.inf).sum(axis=1) == 1).all()
    assert (X[rows["ninf"]] == -np.inf).sum() == 1 and (np.isnan(X[rows["nan"]]).sum(axis=1) == 1).all()
    assert np.isnan(X[rows["allnan"]]).all() and not X[rows["zero"]].any() and X[rows["inf_at_zcol"][0], nf.ZCOL] == np.inf
    assert rows["pinf"] == [0, 63, 64, 255, 256, n - 1] and rows["nan"] == [1, 65, 257]
    assert r1 - r0 >= 64 and (n < 3000 or r1 - r0 >= 1024 + 63)   # a whole wave of a subset that starts in the run; at 3000, aligned waves too
    assert (r1 - r0 > 1024) == (n == 3000)
    with np.errstate(over="ignore"):
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X, equal_nan=True) == f32   # the fp32 rows are the items, or fp64 rows are kept
    assert len(set(fx["qrows"]) & set(fx["bad"])) == 0


@pytest.mark.parametrize("name", nf.NAMES)
def test_scores_of_poisoned_rows(name, oracle_lib):
    fx, ref, V, lqs = oracle(name, oracle_lib)
    assert len(V) == nf.NVEC and (lqs != 0.0).all() and (V[:, nf.ZCOL] == 0.0).all()
    assert np.isfinite(ref.lambdas).all() and not ref.lambdas[fx["bad"]].any()
    for j, q in enumerate(V):
        want = set(fx["nan_rows"]) | ({fx["huge"][j]} if j < len(fx["huge"]) else set())
        for tau in nf.TAUS:
            s = ref.scores(q, tau, lqs[j])
            assert set(np.flatnonzero(np.isnan(s)).tolist()) == want and not np.isinf(s).any()
            term = s[fx["lam_rows"] + [r for h, r in enumerate(fx["huge"]) if h != j]]
            assert np.array_equal(term, np.full(len(term), (1.0 - tau) / (1.0 + abs(lqs[j]))))
            if tau == 1.0:
                assert not nf.bits(term).any()   # +0.0
    for h, r in enumerate(fx["huge"]):   # the overflow is the same in every summation order: two positive terms, the others 0
        t = fx["X"][r] * V[h]
        with np.errstate(over="ignore"):
            assert (t >= 0).all() and (t > 0).sum() == 2 and np.isfinite(t).all() and t.sum() == np.inf
        assert not (fx["X"][r] * np.delete(V, h, axis=0)).any()


def test_the_references_order_nan_as_section_2_says():
    nan, inf = float("nan"), float("inf")
    s = np.array([0.5, nan, -0.0, 0.0, nan, 0.5, -inf])
    assert nf.np_order(np.arange(7), s).tolist() == [0, 5, 2, 3, 6, 1, 4]   # number before NaN, -0.0 ties with +0.0, index ascending
    assert nf.np_order(np.array([9, 3, 7]), np.array([nan, nan, nan]), 2).tolist() == [1, 2]
    S = np.array([[nan, 1.0, nan, 1.2], [2.0, nan, nan, 1.1], [1.0, 3.0, nan, nan]])
    with np.errstate(all="ignore"):
        assert np.array_equal(fused_ref.fuse(S, [1.0, 1.0, 1.0], "max"), [2.0, 3.0, nan, 1.2], equal_nan=True)   # a NaN first, in the middle, last
        assert np.isnan(fused_ref.fuse(S, [1.0, 1.0, 1.0], "sum")).all()
        F = fused_ref.fuse(np.array([[1.1, 1.1, 1.0, 1.0], [1.1, 1.0, 1.1, 1.0]]), [1.7e308, -1.7e308], "sum")
    assert np.isnan(F[0]) and F[1] == inf and F[2] == -inf and F[3] == 0.0
    got = grouped_ref.grouped([0, 1, 2, 3, 4], [7, 7, 8, 8, 9], [nan, 0.3, nan, nan, 0.9], 5, 16)
    assert got == [(9, [(4, 0.9)]), (7, [(1, 0.3)])]   # a NaN item is no member, a group of NaN items does not exist
    m = diverse_ref._margins(np.array([1.0, nan, -inf]), np.array([nan, 0.0, 0.0]), 0.5)
    assert m.tolist() == [-inf, -inf, -inf]


@pytest.mark.parametrize("name", nf.NAMES)
def test_crafted_cases_hold_what_their_names_promise(name, oracle_lib):
    fx, ref, V, lqs = oracle(name, oracle_lib)
    n, topk = fx["X"].shape[0], fx["gp"]["topk"]
    cases = nf.subsets(name)
    assert set(cases) >= {"all", "only poisoned", "one-block mix"} and ("threshold inside the NaN run" in cases) == (n == 3000)
    for j in (0, 5):
        s = ref.scores(V[j], 0.62, lqs[j])
        for case, ids in cases.items():
            assert np.array_equal(ids, np.unique(ids)) and ids.min() >= 0 and ids.max() < n
            numbers = int((~np.isnan(s[ids])).sum())
            if case == "only poisoned":
                assert set(ids.tolist()) <= set(fx["bad"]) and 0 < numbers < min(topk, len(ids)) and len(ids) <= 1024
            if case == "one-block mix":
                assert len(ids) <= 1024 and 0 < numbers < min(topk, len(ids))
            if case == "threshold inside the NaN run":
                assert len(ids) > 1024 and 0 < numbers < topk < len(ids) and set(fx["rows"]["run"]) <= set(ids.tolist())
            if case == "nothing but the NaN run":
                assert len(ids) > 1024 and numbers == 0
    # fused: with the overflowing weights F holds +inf, -inf, NaN out of inf - inf, and finite values
    tau, w = nf.OVERFLOW
    S = np.stack([ref.scores(V[j], tau, lqs[j]) for j in range(3)])
    with np.errstate(all="ignore"):
        F = fused_ref.fuse(S, w, "sum")
    assert (F == np.inf).any() and (F == -np.inf).any() and np.isfinite(F).any() and (np.isnan(F) & ~np.isnan(S).any(axis=0)).any()
    if fx["huge"]:   # a NaN term in the first, the middle and the last vector alone
        assert [np.flatnonzero(np.isnan(S[:, r])).tolist() for r in fx["huge"]] == [[0], [1], [2]]
    assert np.isnan(S[:, fx["nan_rows"]]).all()
    # grouped: group 0 has no member, group 1 ten numbers and ten NaN items
    labels = nf.grouped_labels(fx)["crafted"]
    s = ref.scores(V[0], 0.62, lqs[0])
    assert np.isnan(s[labels == 0]).all() and (labels == 0).sum() == len(fx["rows"]["run"]) - 10
    assert (labels == 1).sum() == 20 and np.isnan(s[labels == 1]).sum() == 10
    assert len(np.unique(nf.grouped_labels(fx)["singletons"])) > 1024 or n < 1024
