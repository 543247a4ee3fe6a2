"""GPU: spherical k-means over the items -- ArrowSpace.assign_cosine, kmeans_spherical, _kmeans_spherical_update, _kmeans_row_scales
 against tests/kmeans_spherical_ref.py, at the tile and segment edges of tests/test_gpu_kmeans.py.
tests/test_kmeans_spherical_inputs.py shows on the CPU the gap that lets the Lloyd runs demand the reference's labels exactly."""
import numpy as np
import pytest

import kmeans_ref as kr
import kmeans_spherical_ref as ks
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
             "dead": lambda: ks.dead_case()[0], "mix": kr.mixture, "grid": ks.grid_mixture}[kind]()
        gp = {"eps": calibrate_eps(np.nan_to_num(X), 4, "l2"), "k": 4, "topk": 4, "p": 2.0, "sigma": None, "metric": "l2", "kernel": "gaussian"}
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
        assert np.array_equal(aspace.get_item(3)[0], X[3])
        _built[key] = (aspace, gl, X)
    return _built[key][0], _built[key][2]


def grid_cap(cap):
    import pyarrowspace_amd as asp
    assert asp._L.as_set_tuning(b"kmeans_grid_cap", cap) == 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_assignment(X, C, labels, cos):
    G, E, rows = ks.cosines(X, C), ks.E(X.shape[1]), np.arange(X.shape[0])
    assert ((labels >= 0) & (labels < C.shape[0])).all()
    print(f"cos: {float(np.abs(cos - G[rows, labels]).max()):.3g} at most, E = {E:.3g}")
    assert (np.abs(cos - G[rows, labels]) <= E).all()
    assert (G[rows, labels] >= G.max(axis=1) - 2.0 * E).all()     # a near-tie: any centroid of the tied set


@pytest.mark.parametrize("n,d,k", CASES)
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_assignment_by_the_largest_cosine(kind, n, d, k):
    aspace, X = space(kind, n, d)
    C = kr.half_centroids(X, k, k) if kind == "int" else kr.jittered_centroids(X, k, 100 + k)
    if k >= 2:
        C[1] = C[0]
    labels, cos = aspace.assign_cosine(C, with_cos=True)
    assert labels.dtype == np.int32 and labels.shape == (n,) and cos.dtype == np.float64 and cos.shape == (n,)
    check_assignment(X, C, labels, cos)
    assert not (labels == 1).any()                                # centroid 1 is centroid 0 again: ties go to the smaller j
    assert np.array_equal(aspace.assign_cosine(C), labels)
    try:
        for cap in (1, 2):   # the later trips of the stride loop: same bits
            grid_cap(cap)
            again, acos = aspace.assign_cosine(C, with_cos=True)
            assert np.array_equal(again, labels) and np.array_equal(bits(acos), bits(cos)), cap
    finally:
        grid_cap(0)


def row_scales(kind):   # the reference's own scales on the grid (pinned); the device's, checked, on fp64 rows
    aspace, X = space(kind)
    w = aspace._kmeans_row_scales()
    with np.errstate(all="ignore"):
        n2 = (X * X).sum(axis=1)
        true = 1.0 / np.sqrt((X.astype(ks.LD) ** 2).sum(axis=1))
    dead = np.isnan(ks.scales(n2))
    if kind == "grid":
        assert np.array_equal(bits(w), bits(ks.scales(n2)))
        return ks.scales(n2)
    assert np.array_equal(np.isnan(w), dead)
    assert (np.abs(w[~dead] - true[~dead]) <= 4 * kr.U * true[~dead]).all()
    return w


@pytest.mark.parametrize("kind", ["grid", "mix"])
def test_update_bits_across_the_segment_edges(kind):
    aspace, X = space(kind)
    labels, C, w = kr.interleaved_labels(), X[:6] + 1.0, row_scales(kind)
    got = aspace._kmeans_spherical_update(labels, C)
    assert np.array_equal(bits(got), bits(ks.update(X, labels, C, w)))
    assert np.array_equal(bits(got[0]), bits(C[0]))               # the empty cluster's centroid is untouched
    with pytest.raises(ValueError, match="label"):
        aspace._kmeans_spherical_update(np.where(labels == 3, 6, labels), C)


def reference_run(kind, which, max_iters):
    key = (kind, which, max_iters)
    if key not in _runs:
        X, inits, _ = ks.lloyd_inputs()[kind]
        _runs[key] = ks.lloyd(X, inits[1 if which == "seed" else 0], row_scales(kind), max_iters)
    return _runs[key]


def check_run(kind, which, max_iters):
    aspace, X = space(kind)
    k = len(kr.MIX_INIT)
    init = {"ids": np.array(kr.MIX_INIT), "array": X[list(kr.MIX_INIT)], "seed": None}[which]
    want = reference_run(kind, which, max_iters)
    c0 = aspace.kmeans_spherical_counters()
    cent, labels, info = aspace.kmeans_spherical(k, init=init, seed=kr.MIX_SEED, max_iters=max_iters, with_info=True)
    c1 = aspace.kmeans_spherical_counters()
    assert np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert (info["iterations"], info["converged"], info["changed"]) == (want["iterations"], want["converged"], want["changed"])
    assert info["counts"].dtype == np.int64 and np.array_equal(info["counts"], want["counts"]) and info["empty"] == want["empty"]
    print(f"cohesion {info['cohesion']:.17g}, reference {want['cohesion']:.17g}")
    assert abs(info["cohesion"] - want["cohesion"]) <= X.shape[0] * (ks.E(X.shape[1]) + kr.U * abs(want["cohesion"]))
    its = info["iterations"]
    ups = its - 1 if info["converged"] else its
    keys = ("calls", "iterations", "assign launches", "update launches", "unit launches", "scale launches", "host waits")
    assert [c1[key] - c0[key] for key in keys] == [1, its, its, 2 * ups, 1 + ups, 1, its + 1]
    return cent, labels, info


@pytest.mark.parametrize("kind,which", [("grid", "ids"), ("grid", "seed"), ("grid", "array"), ("mix", "ids")])
def test_lloyd_runs_equal_the_reference_in_labels_and_centroid_bits(kind, which):
    cent, labels, info = check_run(kind, which, 25)
    assert info["converged"] and info["iterations"] >= 3
    assert np.abs((cent * cent).sum(axis=1) - 1.0).max() <= ks.E(cent.shape[1])
    cent2, labels2, info2 = check_run(kind, which, 2)             # capped: (C_2, labels_2), the labels one step behind
    assert not info2["converged"] and info2["iterations"] == 2 and len(info2["changed"]) == 2
    try:
        for cap in (1, 2):
            grid_cap(cap)
            capped = check_run(kind, which, 25)
            assert np.array_equal(bits(capped[0]), bits(cent)) and np.array_equal(capped[1], labels), cap
            assert bits([capped[2]["cohesion"]])[0] == bits([info["cohesion"]])[0]
    finally:
        grid_cap(0)


def test_dead_rows_are_left_out_of_everything():
    (aspace, X), dead, C, w = space("dead"), list(ks.DEAD_ROWS), ks.dead_case()[1], row_scales("dead")
    assert np.flatnonzero(np.isnan(w)).tolist() == sorted(dead)
    labels, cos = aspace.assign_cosine(C, with_cos=True)
    assert (labels[dead] == -1).all() and np.isnan(cos[dead]).all()
    check_assignment(np.delete(X, dead, axis=0), C, np.delete(labels, dead), np.delete(cos, dead))
    want = ks.lloyd(X, C, w, 3)
    cent, labels, info = aspace.kmeans_spherical(3, init=C, max_iters=3, with_info=True)
    assert (labels[dead] == -1).all() and np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert info["changed"] == want["changed"] and info["changed"][0] == 127 and int(info["counts"].sum()) == 127
    assert np.array_equal(info["counts"], want["counts"]) and np.isfinite(cent).all()
    assert abs(info["cohesion"] - want["cohesion"]) <= 129 * ks.E(33) + 129 * kr.U * abs(want["cohesion"])


def test_refusals_reach_no_kernel():
    aspace, X = space("int", 127, 16)
    c0 = aspace.kmeans_spherical_counters()
    zero = np.vstack([np.ones(16), np.zeros(16)])
    for call in (lambda: aspace.assign_cosine(zero), lambda: aspace.kmeans_spherical(2, init=zero), lambda: aspace.assign_cosine(np.zeros((2, 15))),
                 lambda: aspace.assign_cosine(np.full((2, 16), np.inf)), lambda: aspace.kmeans_spherical(128),
                 lambda: aspace.kmeans_spherical(3, init=[0, 0, 1]), lambda: aspace.kmeans_spherical(3, max_iters=0),
                 lambda: aspace.kmeans_spherical(2, init=np.zeros((3, 16)))):
        with pytest.raises(ValueError):
            call()
    assert aspace.kmeans_spherical_counters() == c0
