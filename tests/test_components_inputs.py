"""CPU: the numpy reference of the connected components (tests/components_ref.py) and the inputs of
tests/test_gpu_components.py, shown with the reference alone.  The union-find agrees with scipy's connected_components (where scipy
imports) and with the synchronous emulation of the device's rounds on every input, with and without thresholds.  The properties the
GPU checks lean on: the scrambled path of 4 099 items (default_rng(7)) is one component that the synchronous rounds connect with 8
lowering rounds (65 537 items: 11), far under the cap of 64; the bridge of `bridged` is the unique largest distance; the ring with
NaN distances splits into three arcs under any threshold; the built shapes A and B of diffuse_ref.SHAPES (on the numpy oracle's
build of the same items) have more than one component and at least one isolated item; every threshold the GPU test places sits in a
relative gap of at least 1e-6 between neighbouring distinct stored distances."""
import numpy as np
import pytest

import components_ref as cr
import diffuse_ref as dfr
import test_gpu_components as tg
from oracle import oracle_np

HAND = ["path", "hubs", "empty", "duplicates", "wide", "bridged", "nan"] + ["ring%dk%d" % (n, k) for n in tg.RING_SIZES for k in (1, 3)]
_graphs = {}


def graph(name):
    """(n, indptr, indices, dist) of an input, once per module: a hand case from its lists, a shape from the numpy oracle's build."""
    if name not in _graphs:
        if name in dfr.SHAPES:
            idx = oracle_np.build(*dfr.shape_items(name))
            _graphs[name] = (len(idx["indptr"]) - 1, np.asarray(idx["indptr"], dtype=np.int64), np.asarray(idx["indices"], dtype=np.int64),
                             np.asarray(idx["dist"], dtype=np.float64))
        else:
            lists = tg.hand_case(name)[2]
            _graphs[name] = (len(lists),) + tg.lists_csr(lists)
    return _graphs[name]


def thresholds(name):
    g = graph(name)
    if cr.distinct_distances(g[3]).shape[0] < 2:
        return [None, np.inf, -np.inf, 1.0]
    return [None, np.inf, -np.inf, float(np.median(g[3][np.isfinite(g[3])]))] + cr.gap_thresholds(g[3], 5)


def scipy_labels(n, indptr, indices, dist, t):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rows, cols = cr.kept_entries(n, indptr, indices, dist, t)
    A = sparse.csr_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(n, n))
    return cr.canonical(connected_components(A, directed=True, connection="weak")[1])


@pytest.mark.parametrize("name", HAND + list(dfr.SHAPES))
def test_the_union_find_against_the_synchronous_rounds(name):
    g = graph(name)
    for t in thresholds(name):
        want = cr.components(*g, t)
        sync, rounds = cr.sync_rounds(*g, t)
        assert np.array_equal(sync, want), (name, t)
        assert rounds <= 12, (name, t)
        assert (want <= np.arange(g[0])).all() and (want[want] == want).all()   # a label is a member, the smallest, and its own label
        i = cr.info(want, *g[1:], t)
        assert i["count"] == np.unique(want).shape[0] and 0 <= i["isolated"] <= i["count"] <= g[0]
        assert i["largest"] == np.bincount(want).max() and (want == i["largest_label"]).sum() == i["largest"]
    # the sweep's warm start: ascending thresholds, each from the last one's labels, end in the cold start's labels
    parent, ts = None, sorted(t for t in thresholds(name) if t is not None)
    for t in ts:
        parent = cr.sync_rounds(*g, t, parent=parent)[0]
        assert np.array_equal(parent, cr.components(*g, t)), (name, t)


@pytest.mark.parametrize("name", HAND + list(dfr.SHAPES))
def test_the_union_find_against_scipy(name):
    g = graph(name)
    for t in thresholds(name):
        assert np.array_equal(cr.components(*g, t), scipy_labels(*g, t)), (name, t)


def test_the_scrambled_path_needs_eight_synchronous_rounds():
    g = graph("path")
    assert g[0] == 4099 == tg.PATH_N and tg.PATH_SEED == 7 and np.diff(g[1]).max() == 2 and g[2].shape[0] == 2 * 4098
    labels, rounds = cr.sync_rounds(*g)
    assert (labels == 0).all() and rounds == 8 and rounds + 1 <= cr.ROUND_CAP == 64
    # the ids carry no order along the path: a propagation of labels alone would walk it
    pos = np.empty(4099, dtype=np.int64)
    pos[np.random.default_rng(7).permutation(4099)] = np.arange(4099)
    assert min(pos[0], 4098 - pos[0]) > 64
    nb = cr.path_lists(65537, 7)
    big = (65537,) + cr.csr_of_lists(65537, nb, [[1.0] * len(x) for x in nb])
    assert cr.sync_rounds(*big)[1] == 11


def test_the_bridge_is_the_unique_largest_distance():
    n, ip, ci, d = graph("bridged")
    n_a, n_b = tg.BRIDGED
    assert n == n_a + n_b and d.max() == 2.0 and (d == d.max()).sum() == 2          # the pair's two stored entries
    rows = np.repeat(np.arange(n), np.diff(ip))
    assert sorted(zip(rows[d == 2.0].tolist(), ci[d == 2.0].tolist())) == [(1, n_a + 1), (n_a + 1, 1)]
    below = 0.5 * (np.sort(d)[-3] + 2.0)
    assert np.sort(d)[-3] < 1.5 and cr.gap_of(d, below) >= 0.1
    assert cr.info(cr.components(n, ip, ci, d), ip, ci, d)["count"] == 1
    assert cr.info(cr.components(n, ip, ci, d, 2.0), ip, ci, d, 2.0)["count"] == 1
    lab = cr.components(n, ip, ci, d, below)
    assert (lab[:n_a] == 0).all() and (lab[n_a:] == n_a).all()


def test_nan_distances_are_kept_only_without_a_threshold():
    n, ip, ci, d = graph("nan")
    assert n == 65 and np.isnan(d).sum() == 2 * len(tg.NAN_PAIRS)
    assert (cr.components(n, ip, ci, d) == 0).all()
    for t in (np.inf, 1e300, float(np.nanmax(d))):
        lab = cr.components(n, ip, ci, d, t)
        assert sorted(set(lab.tolist())) == [0, 11, 31]
    assert np.array_equal(cr.components(n, ip, ci, d, -np.inf), np.arange(n))


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_the_built_shapes_have_components_and_isolated_items(name):
    g = graph(name)
    i = cr.info(cr.components(*g), *g[1:])
    print(f"{name}: {i}")
    assert i["count"] > 1 and i["isolated"] >= 1 and i["largest"] > 1 and i["edges_kept"] == g[2].shape[0]
    assert np.isfinite(g[3]).all() and (g[3] >= 0.0).all()


@pytest.mark.parametrize("name", ["hubs", "duplicates", "wide"] + list(dfr.SHAPES))
def test_every_placed_threshold_sits_in_a_gap(name):
    d = graph(name)[3]
    u = cr.distinct_distances(d)
    for count in (3, 5, 9):
        ts = cr.gap_thresholds(d, count)
        assert len(ts) == count
        for t in ts:
            at = np.searchsorted(u, t)
            assert 0 < at < u.shape[0] and u[at - 1] < t < u[at]
            assert (u[at] - u[at - 1]) >= cr.MIN_GAP * abs(u[at]) and cr.MIN_GAP == 1e-6
    if name in dfr.SHAPES:   # the sweep test's thresholds are distinct
        assert len(set(tg.sweep_thresholds(d))) == 12
