"""CPU: the properties of the inputs tests/test_gpu_kmeans.py leans on, from the reference alone (tests/kmeans_ref.py)."""
import math

import numpy as np
import pytest

import kmeans_ref as kr


@pytest.mark.parametrize("f32", [False, True])
def test_every_assignment_of_the_lloyd_runs_has_a_gap_beyond_the_keys_error(f32):
    """What lets the GPU test demand the reference's labels exactly: at every iteration every item's second-best distance exceeds
    its best by more than 2 max_j E(i, j), with no exception; and the runs are long enough to be cut at two iterations."""
    X = kr.mixture(f32)
    inits = [X[list(kr.MIX_INIT)], X[np.random.default_rng(kr.MIX_SEED).choice(X.shape[0], len(kr.MIX_INIT), replace=False)]]
    worst = []

    def gap(t, C, labels, D):
        two = np.sort(D, axis=1)[:, :2]
        margin = (two[:, 1] - two[:, 0]) - 2.0 * kr.bound(X, C).max(axis=1)
        assert (margin > 0.0).all(), (t, int(margin.argmin()), float(margin.min()))
        worst.append(float(margin.min()))

    for C0 in inits:
        run = kr.lloyd(X, C0, 25, on_assign=gap)
        assert run["converged"] and run["iterations"] >= 3 and run["changed"][0] == X.shape[0] and run["changed"][-1] == 0
    print(f"smallest margin over {len(worst)} assignments: {min(worst):.3g}")


def test_the_nan_case_has_the_same_gap_on_its_finite_rows():
    X, C = kr.nan_case()
    fine = np.arange(X.shape[0]) != kr.NAN_ROW
    assert np.isnan(X[kr.NAN_ROW]).sum() == 1 and np.isfinite(X[fine]).all()

    def gap(t, C, labels, D):
        two = np.sort(D[fine], axis=1)[:, :2]
        assert ((two[:, 1] - two[:, 0]) > 2.0 * kr.bound(X[fine], C).max(axis=1)).all(), t
        assert labels[kr.NAN_ROW] == -1 and (labels[fine] >= 0).all()

    run = kr.lloyd(X, C, 3, on_assign=gap)
    assert run["changed"][0] == 128 and int(run["counts"].sum()) == 128 and np.isfinite(run["centroids"]).all()


def test_update_against_an_exactly_rounded_sum():
    X, labels = kr.mixture(), kr.interleaved_labels()
    assert X.shape[0] == labels.shape[0] and np.bincount(labels[:-1], minlength=6).tolist() == list(kr.SIZES) and labels[-1] == -1
    assert (np.diff(np.flatnonzero(labels == 5)) > 1).any()   # interleaved in id
    C = X[:6] + 1.0
    got = kr.update(X, labels, C)
    assert np.array_equal(got[0], C[0])                       # the empty cluster keeps its centroid
    for j in range(1, 6):
        mem = X[labels == j]
        n = mem.shape[0]
        for c in range(X.shape[1]):
            mean = math.fsum(mem[:, c]) / n
            tol = (n + 1) * kr.U / (1 - (n + 1) * kr.U) * float(np.abs(mem[:, c]).sum()) / n
            assert abs(got[j, c] - mean) <= tol, (j, c)
    assert np.array_equal(got[1], X[labels == 1][0])          # one member: its row, untouched
