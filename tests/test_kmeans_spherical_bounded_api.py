"""CPU: the surface of `ArrowSpace.kmeans_spherical_bounded` and `_kmeans_cos_assign2` -- signatures, docstrings under both module
names, the C entries' null-argument returns -- and the properties of the hard input tests/test_gpu_kmeans_spherical_bounded.py
leans on, from the reference files alone."""
import inspect

import numpy as np

import kmeans_bounded_ref as kbr
import kmeans_spherical_ref as ks

GAP = 1e-9   # against a rounding error of E(33) = 82 * 2^-53 < 1e-14: the device must return the reference's labels exactly


def test_signatures_docstrings_and_bound_entries():
    import arrowspace
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    assert inspect.signature(A.kmeans_spherical_bounded) == inspect.signature(A.kmeans_spherical)
    sig = inspect.signature(A._kmeans_cos_assign2)
    assert list(sig.parameters) == ["self", "centroids", "ids"] and sig.parameters["ids"].default is None
    for mod in (asp, arrowspace):
        for name in ("kmeans_spherical_bounded", "kmeans_spherical_bounded_counters"):
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:"), name
    out = np.zeros(16, dtype=np.int64)
    L, p, EINVAL, err = asp._L, out.ctypes.data, asp._lib.AS_EINVAL, asp._lib.last_error
    assert L.as_kmeans_spherical_bounded(None, p, 1, 1, 1, p, p, p, p, p, p) == EINVAL and "as_kmeans_spherical_bounded: null argument" in err()
    assert L.as_kmeans_cos_assign2(None, p, 1, 1, None, 1, p, p, p) == EINVAL and "as_kmeans_cos_assign2: null argument" in err()
    assert L.as_kmeans_spherical_bounded_counters(None, p, 11) == EINVAL and L.as_kmeans_spherical_bounded_kernel_us(None, 0) == 0.0


def test_the_hard_input_has_a_gap_beyond_the_cosines_error_and_both_skipped_and_active_rows():
    X, ids = kbr.hard()
    n, rows = X.shape[0], np.arange(X.shape[0])
    w = ks.scales((X * X).sum(axis=1))
    worst, active, st = [], [], {}

    def on_assign(t, C, labels, G):
        G = G.astype(np.float64)
        two = np.sort(G, axis=1)[:, -2:]
        worst.append(float((two[:, 1] - two[:, 0]).min()))
        # Hamerly's bound on the chords sqrt(2 - 2 cos) in exact arithmetic: which rows the bound cannot settle
        chord = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * G))
        other = chord.copy()
        other[rows, labels] = np.inf
        lb = other.min(axis=1)
        if t > 1:
            p = np.linalg.norm(C - st["C"], axis=1)
            top = np.argsort(-p, kind="stable")
            kept = st["lb"] - np.where(st["labels"] == top[0], p[top[1]], p[top[0]])
            act = ~(chord[rows, st["labels"]] < kept)
            active.append(int(act.sum()))
            assert np.array_equal(labels[~act], st["labels"][~act])   # a row the bound settles keeps its label
            lb = np.where(act, lb, kept)
        st.update(C=C.copy(), labels=labels, lb=lb)

    run = ks.lloyd(X, X[ids], w, 25, on_assign=on_assign)
    print(f"hard: iterations {run['iterations']}, changed {run['changed']}, smallest gap {min(worst):.3g}, active {active}")
    assert run["iterations"] == 20 and run["converged"] and min(worst) >= GAP
    assert all(0 < a < n for a in active)
