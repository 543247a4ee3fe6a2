"""CPU: the inputs of tests/test_gpu_tail_final_rank.py are what its cases take them for, on the oracle alone
(oracle_np.pair_quantities, fp64): the number P of rows inside eps of every query; the rows inside the ball widened by the largest
error coefficient the coarse scan accepts (4e-2: what its prefilter may append to the candidate buffer) fit the buffer for the
cases that must not overflow, and the ball itself holds more than the buffer for the one that must; exactly one designated
query has P = 0; the tie cases tie exactly; the mass tie ("dups2500") holds more rows than the final kernels' pruned list and,
with everything the prefilter may add, fewer than the candidate buffer."""
import numpy as np
import pytest

import test_gpu_tail_final_rank as tf
from oracle import oracle_np


def _keys(index, group):
    X = tf.make_data()[0]
    prm = oracle_np.resolve_params(tf.graph_params(index))
    q = tf.query_of(group)
    n = np.einsum("ij,ij->i", X, X)
    key, _, _ = oracle_np.pair_quantities(q, X, float(q @ q), n, prm["metric"])
    epskey = oracle_np._eps_key(prm["eps"], prm["metric"])
    # the coarse dot of a row is off by at most coef |x||q|: twice that in a squared distance, that (over |x||q|) in a cosine
    slack = 2.0 * tf.COARSE_COEF_MAX * np.sqrt(n * float(q @ q)) if prm["metric"] == oracle_np.METRIC_L2 else tf.COARSE_COEF_MAX
    return key, epskey, slack


def test_shape_and_groups():
    X, centres, spans = tf.make_data()
    assert X.shape == (tf.NBASE + sum(tf.GROUPS.values()) + tf.HALO * len(tf.GROUPS), tf.D) and X.dtype == np.float64
    assert set(centres) == set(spans) == set(tf.GROUPS)
    np.testing.assert_allclose(np.einsum("ij,ij->i", X, X), 1.0, rtol=1e-12)
    for index, group, tau, fused in tf.CASES:
        assert index in tf.INDEXES and group in tf.GROUPS and 0.4 <= tau <= 1.0
    k = tf.INDEXES["l2"][1]
    assert (tf.GROUPS["lt_k"], tf.GROUPS["eq_k"], tf.GROUPS["k_plus_1"]) == (k - 3, k, k + 1) and 0 < k - 3
    assert tf.GROUPS["dense"] > 1024 and 100 < tf.GROUPS["mid"] < 1024 and tf.GROUPS["crowd"] > tf.CAND_CAP


@pytest.mark.parametrize("index", list(tf.INDEXES))
def test_rows_inside_eps_are_the_cores(index):
    spans = tf.make_data()[2]
    zero = []
    for group, size in tf.GROUPS.items():
        key, epskey, slack = _keys(index, group)
        inside = np.nonzero(key <= epskey)[0]
        lo, m = spans[group]
        assert len(inside) == size and (size == 0 or (inside[0] == lo and inside[-1] == lo + m - 1)), (index, group, len(inside))
        # no row sits within rounding of the bound: P does not depend on how a key is summed
        assert np.abs(key - epskey).min() > 1e-9 * epskey
        wide = int((key <= epskey + slack).sum())
        if group == "crowd":
            assert len(inside) > tf.CAND_CAP
        else:
            assert wide <= tf.CAND_CAP, (index, group, wide)
        if len(inside) == 0:
            zero.append(group)
    assert zero == [tf.ZERO_GROUP]


@pytest.mark.parametrize("index", ["l2", "cosine"])
def test_tie_cases_tie(index):
    spans = tf.make_data()[2]
    for g in ("dups", "dups100", "dups2500"):
        key, epskey, _ = _keys(index, g)
        lo, m = spans[g]
        assert len(np.unique(key[lo:lo + m])) == 1                  # every key equal: kmax == kmin
    assert tf.GROUPS["dups"] <= 64 < tf.GROUPS["dups100"]           # (on either side of what is ranked without the selection)
    # the mass tie: 2 500 rows inside eps, all on the query (cosine 1: every score in one bin), more than the pruned list holds,
    # and with the halo and whatever the coarse prefilter may add fewer than the candidate buffer
    key, epskey, slack = _keys(index, "dups2500")
    lo, m = spans["dups2500"]
    X = tf.make_data()[0]
    assert m == tf.GROUPS["dups2500"] == 2500 > tf.PRUNE_CAP and int((key <= epskey).sum()) == 2500
    assert (X[lo:lo + m] == tf.query_of("dups2500")[None, :]).all()
    assert int((key <= epskey + slack).sum()) < tf.CAND_CAP and m + tf.HALO < tf.CAND_CAP
    key, epskey, _ = _keys(index, "pairs")
    lo, m = spans["pairs"]
    kk = key[lo:lo + m]
    np.testing.assert_array_equal(kk[: m // 2], kk[m // 2:])        # each key twice: ids decide
    assert len(np.unique(kk)) == m // 2
    order = np.lexsort((np.arange(m), kk))
    assert kk[order[0]] == kk[order[1]] and order[0] < order[1]     # (k = 1, index "l2_k1": the cut falls inside a pair)


def test_cases_cover_what_the_issue_lists():
    by_index = {}
    for index, group, tau, fused in tf.CASES:
        by_index.setdefault(index, set()).add(group)
    assert {"none", "lt_k", "eq_k", "k_plus_1", "mid", "dense", "pairs", "dups", "dups100"} <= by_index["l2"]
    assert {"none", "mid", "dense", "pairs", "dups", "dups100"} <= by_index["cosine"]
    assert by_index["l2_crowd"] == by_index["cosine_crowd"] == {"crowd"}
    assert tf.INDEXES["l2_crowd"] == tf.INDEXES["l2"] and tf.INDEXES["cosine_crowd"] == tf.INDEXES["cosine"]
    assert by_index["l2_dups2500"] == by_index["cosine_dups2500"] == {"dups2500"}
    assert tf.INDEXES["l2_dups2500"] == tf.INDEXES["l2"] and tf.INDEXES["cosine_dups2500"] == tf.INDEXES["cosine"]
    assert list(tf.GROUPS)[-1] == "dups2500"      # appended: the generator draws in order, the groups before it keep their rows
    assert ("l2_dups2500", "dups2500", 0.62, False) in tf.CASES and ("cosine_dups2500", "dups2500", 0.62, False) in tf.CASES
    assert tf.INDEXES["l2_k1"][1:] == (1, 1) and tf.INDEXES["l2_k120"][1] == 120
    assert tf.INDEXES["l2_topk500"][2] > tf.GROUPS["lt_k"] + tf.HALO      # more hits asked for than the query's own group holds
    assert sum(group == tf.ZERO_GROUP for index, group, tau, fused in tf.CASES if index == "l2") == 1
