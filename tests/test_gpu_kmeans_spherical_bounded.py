"""GPU: bound-pruned spherical k-means -- ArrowSpace.kmeans_spherical_bounded, _kmeans_cos_assign2 against
tests/kmeans_spherical_ref.py and against kmeans_spherical on the same index.  The assignment kernel keeps kms_assign_kernel's
128 x 64 x 32 tile, so the shapes and id lists are those of tests/test_gpu_kmeans_bounded.py; the indexes are shared with
tests/test_gpu_kmeans_spherical.py.  tests/test_kmeans_spherical_bounded_api.py shows on the CPU the gap that lets the run on the
hard input demand the reference's labels exactly."""
import numpy as np
import pytest

import kmeans_ref as kr
import kmeans_spherical_ref as ks
from test_gpu_kmeans_bounded import CASES, grid_caps, inputs
from test_gpu_kmeans_spherical import bits, row_scales, space

pytestmark = pytest.mark.gpu

SAME = ("iterations", "converged", "changed", "empty")
_runs = {}


@pytest.mark.parametrize("n,d,k", CASES)
def test_cos_assign2_over_id_lists_carries_the_bits_of_assign_cosine(n, d, k):
    aspace, X = space("gauss", n, d)
    C = kr.jittered_centroids(X, k, 100 + k)
    flabels, fcos = aspace.assign_cosine(C, with_cos=True)
    G = ks.cosines(X, C)
    G[np.arange(n), flabels] = -np.inf
    wsecond = G.max(axis=1)                                       # longdouble, over the centroids other than the label
    for m in (1, 127, 128, 129):
        ids = np.random.default_rng(m).integers(0, n, m)
        ids[-1] = ids[0]   # (m > 1: a repeat for certain)
        first = None
        for cap in grid_caps((0, 1, 2)):
            labels, cos, second = aspace._kmeans_cos_assign2(C, ids)
            assert labels.dtype == np.int32 and labels.shape == cos.shape == second.shape == (m,)
            assert np.array_equal(labels, flabels[ids]) and np.array_equal(bits(cos), bits(fcos[ids])), (m, cap)
            if k == 1:
                assert np.isneginf(second).all()
                continue
            print(f"m {m} cap {cap}: second off by {float(np.abs(second - wsecond[ids]).max()):.3g} at most, 2 E = {2 * ks.E(d):.3g}")
            assert (np.abs(second - wsecond[ids]) <= 2 * ks.E(d)).all(), (m, cap)
            first = second if first is None else first
            assert np.array_equal(bits(second), bits(first)), (m, cap)


def run_inputs(kind):
    """-> (ArrowSpace, X, the starting ids, the row scales the reference runs with) of "grid", "mix" and "hard"."""
    if kind != "hard":
        return space(kind) + (np.array(kr.MIX_INIT), row_scales(kind))
    aspace, X, ids = inputs("hard")
    w, true = aspace._kmeans_row_scales(), 1.0 / np.sqrt((X.astype(ks.LD) ** 2).sum(axis=1))
    assert (np.abs(w - true) <= 4 * kr.U * true).all()            # fp64 rows: the device's scales, checked (as row_scales)
    return aspace, X, ids, w


def expected(kind, max_iters):
    """The reference's run and kmeans_spherical's on the same index, once per (kind, max_iters)."""
    if (kind, max_iters) not in _runs:
        aspace, X, ids, w = run_inputs(kind)
        _runs[kind, max_iters] = (ks.lloyd(X, X[ids], w, max_iters), aspace.kmeans_spherical(len(ids), init=ids, max_iters=max_iters, with_info=True))
    return _runs[kind, max_iters]


def check_run(kind, max_iters):
    aspace, X, ids, _ = run_inputs(kind)
    want, (pcent, plabels, pinfo) = expected(kind, max_iters)
    c0 = aspace.kmeans_spherical_bounded_counters()
    cent, labels, info = aspace.kmeans_spherical_bounded(len(ids), init=ids, max_iters=max_iters, with_info=True)
    c1 = aspace.kmeans_spherical_bounded_counters()
    assert np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert [info[key] for key in SAME] == [want[key] for key in SAME] == [pinfo[key] for key in SAME]
    assert info["counts"].dtype == np.int64 and np.array_equal(info["counts"], want["counts"]) and np.array_equal(info["counts"], pinfo["counts"])
    assert np.array_equal(labels, plabels) and np.array_equal(bits(cent), bits(pcent))
    print(f"cohesion {info['cohesion']:.17g}, reference {want['cohesion']:.17g}; active {info['active']}")
    assert abs(info["cohesion"] - want["cohesion"]) <= X.shape[0] * (ks.E(X.shape[1]) + kr.U * abs(want["cohesion"]))
    its, active = info["iterations"], info["active"]
    assert len(active) == its and active[0] == X.shape[0] and all(0 <= a <= X.shape[0] for a in active)
    assert all(ch <= a for ch, a in zip(info["changed"], active))
    ups = its - 1 if info["converged"] else its
    names = ("calls", "iterations", "assign launches", "update launches", "unit launches", "scale launches", "filter launches", "shift launches",
             "host waits", "active rows")
    assert [c1[key] - c0[key] for key in names] == [1, its, its, 2 * ups, 1 + ups, 1, its - 1, its - 1, its + 1, sum(active)]
    return cent, labels, info


@pytest.mark.parametrize("kind", ["grid", "mix", "hard"])
def test_bounded_runs_equal_the_reference_and_kmeans_spherical_in_labels_and_centroid_bits(kind):
    cent, labels, info = check_run(kind, 25)
    assert info["converged"] and info["iterations"] >= 3
    if kind == "hard":
        assert info["iterations"] == 20 and all(0 < a < labels.shape[0] for a in info["active"][1:])
    _, _, info2 = check_run(kind, 2)   # capped: (C_2, labels_2)
    assert not info2["converged"] and info2["iterations"] == 2 and len(info2["active"]) == 2
    for cap in grid_caps():
        capped = check_run(kind, 25)
        assert np.array_equal(bits(capped[0]), bits(cent)) and np.array_equal(capped[1], labels), cap
        assert bits([capped[2]["cohesion"]])[0] == bits([info["cohesion"]])[0] and capped[2]["active"] == info["active"], cap


def test_dead_rows_are_never_active():
    (aspace, X), dead, C, w = space("dead"), list(ks.DEAD_ROWS), ks.dead_case()[1], row_scales("dead")
    labels, cos, second = aspace._kmeans_cos_assign2(C, [dead[0], 0, dead[1]])
    assert labels[0] == labels[2] == -1 and labels[1] >= 0 and np.isnan(cos[[0, 2]]).all() and np.isnan(second[[0, 2]]).all()
    want = ks.lloyd(X, C, w, 3)
    cent, labels, info = aspace.kmeans_spherical_bounded(3, init=C, max_iters=3, with_info=True)
    assert (labels[dead] == -1).all() and np.array_equal(labels, want["labels"]) and np.array_equal(bits(cent), bits(want["centroids"]))
    assert info["changed"] == want["changed"] and info["changed"][0] == 127 and np.array_equal(info["counts"], want["counts"])
    assert info["active"][0] == 129 and all(a <= 127 for a in info["active"][1:])
    assert abs(info["cohesion"] - want["cohesion"]) <= 129 * ks.E(33) + 129 * kr.U * abs(want["cohesion"]) and np.isfinite(cent).all()


def test_refusals_reach_no_kernel():
    aspace, X = space("int", 127, 16)
    c0 = aspace.kmeans_spherical_bounded_counters()
    zero = np.vstack([np.ones(16), np.zeros(16)])
    for call in (lambda: aspace._kmeans_cos_assign2(zero), lambda: aspace.kmeans_spherical_bounded(2, init=zero),
                 lambda: aspace._kmeans_cos_assign2(np.zeros((2, 15))), lambda: aspace._kmeans_cos_assign2(np.full((2, 16), np.inf)),
                 lambda: aspace._kmeans_cos_assign2(np.ones((2, 16)), [0, 127]), lambda: aspace.kmeans_spherical_bounded(128),
                 lambda: aspace.kmeans_spherical_bounded(3, init=[0, 0, 1]), lambda: aspace.kmeans_spherical_bounded(3, max_iters=0),
                 lambda: aspace.kmeans_spherical_bounded(2, init=np.zeros((3, 16)))):
        with pytest.raises(ValueError):
            call()
    assert aspace.kmeans_spherical_bounded_counters() == c0
