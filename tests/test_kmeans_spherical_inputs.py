"""CPU: the properties of the inputs tests/test_gpu_kmeans_spherical.py leans on, from tests/kmeans_spherical_ref.py alone."""
import numpy as np
import pytest

import kmeans_spherical_ref as ks

GAP = 1e-9   # against a rounding error of E(33) = 82 * 2^-53 < 1e-14: the device must return the reference's labels exactly


def test_the_grid_mixture_pins_its_row_scales():
    X = ks.grid_mixture()
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    exact = (np.round(X * 1024).astype(np.int64) ** 2).sum(axis=1)            # integers below 2^53: exact in any order
    assert exact.max() < 2 ** 53 and np.array_equal((X * X).sum(axis=1) * 2.0 ** 20, exact.astype(np.float64))
    assert np.isfinite(ks.scales((X * X).sum(axis=1))).all()


@pytest.mark.parametrize("name", ["grid", "mix", "dead"])
def test_every_assignment_of_the_lloyd_runs_has_a_gap_beyond_the_cosines_error(name):
    X, inits, max_iters = ks.lloyd_inputs()[name]
    with np.errstate(all="ignore"):
        w = ks.scales((X * X).sum(axis=1))
    live, worst = ~np.isnan(w), []

    def gap(t, C, labels, G):
        two = np.sort(G[live].astype(np.float64), axis=1)[:, -2:]
        worst.append(float((two[:, 1] - two[:, 0]).min()))
        assert worst[-1] >= GAP, (t, worst[-1])

    runs = [ks.lloyd(X, C0, w, max_iters, on_assign=gap) for C0 in inits]
    print(f"{name}: iterations {[r['iterations'] for r in runs]}, smallest gap {min(worst):.3g}")
    if name == "dead":
        assert np.flatnonzero(~live).tolist() == sorted(ks.DEAD_ROWS) and int(runs[0]["counts"].sum()) == X.shape[0] - 2
    else:
        assert all(r["converged"] and r["iterations"] >= 3 for r in runs)
    assert name != "grid" or [r["iterations"] for r in runs] == [10, 14]
