"""GPU: k-means over the items -- ArrowSpace.assign, kmeans, _kmeans_update against tests/kmeans_ref.py.
The assign kernel's tiles are 128 rows x 64 centroids x 32 columns, so the shapes are one below, at and one above each edge:
n in {127, 128, 129, 257}, d in {16, 32, 33, 70}, k in {1, 2, 63, 64, 65, 130}, a sparse pairing (CASES), not the product; the
update's segment of 256 members is crossed by the cluster sizes 0, 1, 255, 256, 257 and 513 of kmeans_ref.interleaved_labels().
Indexes follow the clustered / calibrate_eps recipe of tests/test_gpu_diffuse.py; tests/test_kmeans_inputs.py shows on the CPU the
gap that lets the Lloyd runs demand the reference's labels exactly."""
import numpy as np
import pytest

import kmeans_ref as kr
from conftest import calibrate_eps

pytestmark = pytest.mark.gpu

CASES = [(127, 16, 1), (127, 16, 64), (128, 32, 2), (128, 32, 65), (129, 33, 63), (129, 33, 130), (257, 70, 64), (257, 70, 130), (257, 70, 1)]
_built, _runs = {}, {}


def space(kind, n=0, d=0):
    """One index per (kind, shape) for the whole module -> (ArrowSpace, the items it stores)."""
    import pyarrowspace_amd as asp
    key = (kind, n, d)
    if key not in _built:
        X = {"int": lambda: kr.integer_items(n, d, n + d), "gauss": lambda: kr.gaussian_items(n, d, n + d),
             "nan": lambda: kr.nan_case()[0], "mix": kr.mixture, "mix32": lambda: kr.mixture(True)}[kind]()
        gp = {"eps": calibrate_eps(np.nan_to_num(X), 4, "l2"), "k": 4, "topk": 4, "p": 2.0, "sigma": None, "metric": "l2", "kernel": "gaussian"}
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        assert np.array_equal(aspace.get_item(3)[0], X[3])
        _built[key] = (aspace, gl, X, asp)
    return _built[key][0], _built[key][2]


def grid_cap(cap):
    import pyarrowspace_amd as asp
    assert asp._L.as_set_tuning(b"kmeans_grid_cap", cap) == 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,d,k", CASES)
def test_exact_assignment_on_integer_items(n, d, k):
    aspace, X = space("int", n, d)
    C = kr.half_centroids(X, k, k)
    want, wdist, D = kr.assign(X, C)
    labels, dist = aspace.assign(C, with_dist=True)
    assert labels.dtype == np.int32 and labels.shape == (n,) and dist.dtype == np.float64
    assert np.array_equal(labels, want) and np.array_equal(dist, wdist)
    if k >= 2:
        assert not (labels == 1).any()                               # centroid 1 is centroid 0 again: ties go to the smaller j
    if k >= 4:
        assert D[5, 2] == D[5, 3] == 0.25 and labels[5] == 2 and dist[5] == 0.25
    assert np.array_equal(aspace.assign(C), labels)


def check_rounded(X, C, labels, dist):
    D, E = kr.dists(X, C), kr.bound(X, C)
    rows = np.arange(X.shape[0])
    assert ((labels >= 0) & (labels < C.shape[0])).all()
    print(f"dist: {np.abs(dist - D[rows, labels]).max():.3g} at most, E >= {E.min():.3g}")
    assert (np.abs(dist - D[rows, labels]) <= E[rows, labels]).all()
    assert (D[rows, labels] <= D.min(axis=1) + 2.0 * E.max(axis=1)).all()   # a near-tie: any centroid of the tied set


@pytest.mark.parametrize("n,d,k", CASES)
def test_rounded_assignment_on_fp64_items(n, d, k):
    aspace, X = space("gauss", n, d)
    C = kr.jittered_centroids(X, k, 100 + k)
    labels, dist = aspace.assign(C, with_dist=True)
    check_rounded(X, C, labels, dist)
    try:
        for cap in (1, 2):   # the later trips of the stride loop: same bits
            grid_cap(cap)
            again, adist = aspace.assign(C, with_dist=True)
            assert np.array_equal(again, labels) and np.array_equal(bits(adist), bits(dist)), cap
    finally:
        grid_cap(0)


@pytest.mark.parametrize("kind", ["mix", "mix32"])
def test_update_bits_across_the_segment_edges(kind):
    aspace, X = space(kind)
    labels = kr.interleaved_labels()
    C = X[:6] + 1.0
    got = aspace._kmeans_update(labels, C)
    assert np.array_equal(bits(got), bits(kr.update(X, labels, C)))
    assert np.array_equal(bits(got[0]), bits(C[0]))                  # the empty cluster's centroid is untouched
    with pytest.raises(ValueError, match="label"):
        aspace._kmeans_update(np.where(labels == 3, 6, labels), C)


def reference_run(kind, which, max_iters):
    key = (kind, which, max_iters)
    if key not in _runs:
        X = space(kind)[1]
        ids = list(kr.MIX_INIT) if which != "seed" else np.random.default_rng(kr.MIX_SEED).choice(X.shape[0], len(kr.MIX_INIT), replace=False)
        _runs[key] = kr.lloyd(X, X[ids], max_iters)
    return _runs[key]


def check_run(kind, which, max_iters):
    aspace, X = space(kind)
    k = len(kr.MIX_INIT)
    init = {"ids": np.array(kr.MIX_INIT), "array": X[list(kr.MIX_INIT)], "seed": None}[which]
    want = reference_run(kind, which, max_iters)
    c0 = aspace.kmeans_counters()
    cent, labels, info = aspace.kmeans(k, init=init, seed=kr.MIX_SEED, max_iters=max_iters, with_info=True)
    c1 = aspace.kmeans_counters()
    assert np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert (info["iterations"], info["converged"], info["changed"]) == (want["iterations"], want["converged"], want["changed"])
    assert info["counts"].dtype == np.int64 and np.array_equal(info["counts"], want["counts"]) and info["empty"] == want["empty"]
    live = labels >= 0
    E = kr.bound(X[live], want["centroids"] if want["converged"] else reference_run(kind, which, max_iters - 1)["centroids"])
    tol = E[np.arange(int(live.sum())), labels[live]].sum() + X.shape[0] * kr.U * want["inertia"]
    print(f"inertia {info['inertia']:.17g}, reference {want['inertia']:.17g}, bound {tol:.3g}")
    assert abs(info["inertia"] - want["inertia"]) <= tol
    its = info["iterations"]
    assert [c1[key] - c0[key] for key in ("calls", "iterations", "assign launches", "host waits")] == [1, its, its, its + 1]
    return cent, labels, info


@pytest.mark.parametrize("kind,which", [("mix", "ids"), ("mix", "array"), ("mix", "seed"), ("mix32", "ids")])
def test_lloyd_runs_equal_the_reference_in_labels_and_centroid_bits(kind, which):
    cent, labels, info = check_run(kind, which, 25)
    assert info["converged"] and info["iterations"] >= 3
    plain = space(kind)[0].kmeans(len(kr.MIX_INIT), init=np.array(kr.MIX_INIT), seed=kr.MIX_SEED) if which == "ids" else None
    assert plain is None or (np.array_equal(bits(plain[0]), bits(cent)) and np.array_equal(plain[1], labels))
    cent2, labels2, info2 = check_run(kind, which, 2)                # capped: (C_2, labels_2), the labels one step behind
    assert not info2["converged"] and info2["iterations"] == 2 and len(info2["changed"]) == 2
    try:
        for cap in (1, 2):
            grid_cap(cap)
            capped = check_run(kind, which, 25)
            assert np.array_equal(bits(capped[0]), bits(cent)) and np.array_equal(capped[1], labels), cap
            assert bits([capped[2]["inertia"]])[0] == bits([info["inertia"]])[0]
    finally:
        grid_cap(0)


def test_an_item_with_a_nan_is_left_out_of_everything():
    aspace, X = space("nan", 129, 33)
    r, C = kr.NAN_ROW, kr.nan_case()[1]
    labels, dist = aspace.assign(C, with_dist=True)
    assert labels[r] == -1 and np.isnan(dist[r]) and (np.delete(labels, r) >= 0).all()
    check_rounded(np.delete(X, r, axis=0), C, np.delete(labels, r), np.delete(dist, r))
    want = kr.lloyd(X, C, 3)
    cent, labels, info = aspace.kmeans(3, init=C, max_iters=3, with_info=True)
    assert labels[r] == -1 and np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert info["changed"] == want["changed"] and info["changed"][0] == 128 and int(info["counts"].sum()) == 128
    assert np.array_equal(info["counts"], want["counts"]) and np.isfinite(info["inertia"]) and np.isfinite(cent).all()


def test_refusals_reach_no_kernel():
    aspace, X = space("int", 127, 16)
    c0 = aspace.kmeans_counters()
    for call in (lambda: aspace.assign(np.zeros((2, 15))), lambda: aspace.assign(np.full((2, 16), np.inf)), lambda: aspace.kmeans(128),
                 lambda: aspace.kmeans(3, init=[0, 0, 1]), lambda: aspace.kmeans(3, max_iters=0), lambda: aspace.kmeans(2, init=np.zeros((3, 16)))):
        with pytest.raises(ValueError):
            call()
    assert aspace.kmeans_counters() == c0
