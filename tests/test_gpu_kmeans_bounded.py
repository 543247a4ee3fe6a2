"""GPU: bound-pruned Lloyd iterations -- ArrowSpace.kmeans_bounded, _kmeans_assign2 against tests/kmeans_ref.py and
tests/kmeans_bounded_ref.py.  The assignment kernel keeps km_assign_kernel's 128 x 64 x 32 tile, so the shapes are a sparse subset
of tests/test_gpu_kmeans.py's CASES (whose indexes are shared); the id lists are one below, at and one above a tile of rows."""
import numpy as np
import pytest

import kmeans_bounded_ref as kbr
import kmeans_ref as kr
from conftest import calibrate_eps
from test_gpu_kmeans import bits, space

pytestmark = pytest.mark.gpu

CASES = [(127, 16, 1), (127, 16, 64), (128, 32, 65), (129, 33, 130), (257, 70, 64)]
_hard, _runs = [], {}


def grid_caps(caps=(1, 2)):
    """The later trips of the kernels' stride loops."""
    import pyarrowspace_amd as asp
    try:
        for cap in caps:
            assert asp._L.as_set_tuning(b"kmeans_bounded_grid_cap", cap) == 0
            yield cap
    finally:
        asp._L.as_set_tuning(b"kmeans_bounded_grid_cap", 0)


def inputs(kind):
    """-> (ArrowSpace, X, the starting ids) of the runs "mix", "mix32" and "hard"."""
    if kind != "hard":
        return space(kind) + (np.array(kr.MIX_INIT),)
    if not _hard:
        import pyarrowspace_amd as asp
        X, ids = kbr.hard()
        gp = {"eps": calibrate_eps(X, 4, "l2"), "k": 4, "topk": 4, "p": 2.0, "sigma": None, "metric": "l2", "kernel": "gaussian"}
        _hard.extend([asp.ArrowSpaceBuilder.build(gp, X), X, ids])
    return _hard[0][0], _hard[1], _hard[2]


def reference_run(kind, max_iters):
    if (kind, max_iters) not in _runs:
        _, X, ids = inputs(kind)
        _runs[kind, max_iters] = kr.lloyd(X, X[ids], max_iters)
    return _runs[kind, max_iters]


@pytest.mark.parametrize("n,d,k", CASES)
def test_assign2_is_exact_on_integer_items(n, d, k):
    aspace, X = space("int", n, d)
    C = kr.half_centroids(X, k, k)
    want, wdist, _ = kr.assign(X, C)
    labels, dist, second = aspace._kmeans_assign2(C)
    assert labels.dtype == np.int32 and labels.shape == dist.shape == second.shape == (n,)
    assert np.array_equal(labels, want) and np.array_equal(dist, wdist) and np.array_equal(second, kbr.second(X, C, want))
    if k >= 2:
        assert not (labels == 1).any() and np.array_equal(second[labels == 0], dist[labels == 0])   # centroid 1 is centroid 0 again
    else:
        assert np.isposinf(second).all()


@pytest.mark.parametrize("n,d,k", CASES)
def test_assign2_over_id_lists_carries_the_bits_of_assign(n, d, k):
    aspace, X = space("gauss", n, d)
    C = kr.jittered_centroids(X, k, 100 + k)
    flabels, fdist = aspace.assign(C, with_dist=True)
    wsecond, E = kbr.second(X, C, flabels), kr.bound(X, C).max(axis=1)
    for m in (1, 127, 128, 129):
        ids = np.random.default_rng(m).integers(0, n, m)
        ids[-1] = ids[0]   # (m > 1: a repeat for certain)
        first = None
        for cap in grid_caps((0, 1, 2)):
            labels, dist, second = aspace._kmeans_assign2(C, ids)
            assert np.array_equal(labels, flabels[ids]) and np.array_equal(bits(dist), bits(fdist[ids])), (m, cap)
            if k == 1:
                assert np.isposinf(second).all() and np.isposinf(wsecond).all()
                continue
            print(f"m {m} cap {cap}: second off by {np.abs(second - wsecond[ids]).max():.3g} at most, E >= {E.min():.3g}")
            assert (np.abs(second - wsecond[ids]) <= E[ids]).all(), (m, cap)
            first = second if first is None else first
            assert np.array_equal(bits(second), bits(first)), (m, cap)


def check_run(kind, max_iters):
    aspace, X, ids = inputs(kind)
    want = reference_run(kind, max_iters)
    c0 = aspace.kmeans_bounded_counters()
    cent, labels, info = aspace.kmeans_bounded(len(ids), init=ids, max_iters=max_iters, with_info=True)
    c1 = aspace.kmeans_bounded_counters()
    assert np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert (info["iterations"], info["converged"], info["changed"]) == (want["iterations"], want["converged"], want["changed"])
    assert info["counts"].dtype == np.int64 and np.array_equal(info["counts"], want["counts"]) and info["empty"] == want["empty"]
    live = labels >= 0   # the bound of tests/test_gpu_kmeans.py's check_run
    E = kr.bound(X[live], want["centroids"] if want["converged"] else reference_run(kind, max_iters - 1)["centroids"])
    tol = E[np.arange(int(live.sum())), labels[live]].sum() + X.shape[0] * kr.U * want["inertia"]
    print(f"inertia {info['inertia']:.17g}, reference {want['inertia']:.17g}, bound {tol:.3g}; active {info['active']}")
    assert abs(info["inertia"] - want["inertia"]) <= tol
    its, active = info["iterations"], info["active"]
    assert len(active) == its and active[0] == X.shape[0] and all(0 <= a <= X.shape[0] for a in active)
    assert all(ch <= a for ch, a in zip(info["changed"], active))
    names = ("calls", "iterations", "assign launches", "filter launches", "shift launches", "host waits", "active rows")
    assert [c1[key] - c0[key] for key in names] == [1, its, its, its - 1, its - 1, its + 1, sum(active)]
    return cent, labels, info


@pytest.mark.parametrize("kind", ["mix", "mix32", "hard"])
def test_bounded_runs_equal_the_reference_in_labels_and_centroid_bits(kind):
    cent, labels, info = check_run(kind, 25)
    assert info["converged"] and info["iterations"] >= 3
    if kind == "hard":
        assert info["iterations"] == 20 and all(0 < a < labels.shape[0] for a in info["active"][1:])
    _, _, info2 = check_run(kind, 2)   # capped: (C_2, labels_2)
    assert not info2["converged"] and info2["iterations"] == 2 and len(info2["active"]) == 2
    for cap in grid_caps():
        capped = check_run(kind, 25)
        assert np.array_equal(bits(capped[0]), bits(cent)) and np.array_equal(capped[1], labels), cap
        assert bits([capped[2]["inertia"]])[0] == bits([info["inertia"]])[0] and capped[2]["active"] == info["active"], cap


def test_an_item_with_a_nan_never_becomes_active():
    aspace, X = space("nan", 129, 33)
    r, C = kr.NAN_ROW, kr.nan_case()[1]
    labels, dist, second = aspace._kmeans_assign2(C, [r, 0, r])
    assert labels[0] == labels[2] == -1 and labels[1] >= 0 and np.isnan(dist[[0, 2]]).all() and np.isnan(second[[0, 2]]).all()
    want = kr.lloyd(X, C, 3)
    cent, labels, info = aspace.kmeans_bounded(3, init=C, max_iters=3, with_info=True)
    assert labels[r] == -1 and np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert info["changed"] == want["changed"] and info["changed"][0] == 128 and np.array_equal(info["counts"], want["counts"])
    assert info["active"][0] == 129 and all(a <= 128 for a in info["active"][1:])
    assert np.isfinite(info["inertia"]) and np.isfinite(cent).all()


def test_refusals_reach_no_kernel():
    aspace, X = space("int", 127, 16)
    c0 = aspace.kmeans_bounded_counters()
    for call in (lambda: aspace._kmeans_assign2(np.zeros((2, 15))), lambda: aspace._kmeans_assign2(np.full((2, 16), np.inf)),
                 lambda: aspace._kmeans_assign2(np.zeros((2, 16)), [0, 127]), lambda: aspace.kmeans_bounded(128),
                 lambda: aspace.kmeans_bounded(3, init=[0, 0, 1]), lambda: aspace.kmeans_bounded(3, max_iters=0),
                 lambda: aspace.kmeans_bounded(2, init=np.zeros((3, 16)))):
        with pytest.raises(ValueError):
            call()
    assert aspace.kmeans_bounded_counters() == c0
