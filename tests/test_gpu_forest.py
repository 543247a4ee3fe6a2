"""GPU: the minimum spanning forest of the item graph -- ArrowSpace.spanning_forest and the C entry behind it.
Every expected edge comes from tests/forest_ref.py (Kruskal under S23's total order) on the CSR the device itself stores, and the
cuts are compared with `components` on the same graph; `rounds` depends on nothing but the graph either, and is bounded.  The
hand-built graphs are those of tests/test_gpu_components.py and two of forest_ref; the built shapes are test_gpu_diffuse.py's."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import components_ref as cr
import diffuse_ref as dfr
import forest_ref as fr
import test_gpu_graph_stage as gs
from conftest import calibrate_feature_eps, clustered
from test_gpu_components import RING_SIZES, Hand, hand_case, lists_csr, shape_csr
from test_gpu_diffuse import Index, _built, index

pytestmark = pytest.mark.gpu

HAND = (["path", "hubs", "empty"] + ["ring%dk%d" % (n, k) for n in RING_SIZES for k in (1, 2)]
        + ["duplicates", "wide", "bridged", "nan", "twoway", "monotone"])
_cases = {}


def forest_case(name):
    """-> (X, graph parameters, lists): `hand_case`, or one of forest_ref's inputs with its made-up dists in the lists."""
    if name not in ("twoway", "monotone"):
        return hand_case(name)
    nbrs, dists = getattr(fr, name)()
    X = clustered(len(nbrs), gs.D, nclust=6, seed=43)
    _, lists = gs.lists_from_neighbours(X, "l2", nbrs)
    gp = gs.graph_params("l2", "gaussian", 2.0, 2, lists)   # (sigma from the items' own distances: a made-up one is a NaN)
    made = [dict(zip(js, ds)) for js, ds in zip(nbrs, dists)]
    return X, gp, [(js, key, np.array([made[i][int(j)] for j in js], dtype=np.float64), gy) for i, (js, key, _, gy) in enumerate(lists)]


class ForestHand(Hand):
    """`Hand` for the cases of `forest_case` (its constructor reads `hand_case` alone, so the steps are restated here), with the
    forest call on the engine's handles."""

    def __init__(self, name):
        X, gp, lists = forest_case(name)
        self.e = gs._engine(gp, X)
        self.e.graph_from_knn(*[gs._dev(a) for a in gs.pack_lists(lists, gp["k"])])
        self.L, self.n = self.e.L, X.shape[0]
        nnz = int(self.L.as_graph_nnz(self.e.gr)) - self.n
        ip, ix, dd = np.zeros(self.n + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64), np.zeros(max(nnz, 1))
        self.e._check(self.L.as_graph_csr_dist(self.e.gr, ip.ctypes.data, ix.ctypes.data, dd.ctypes.data))
        self.csr = (ip, ix[:nnz], dd[:nnz])
        want = lists_csr(lists)   # the structure is the lists', both directions
        assert ip[self.n] == nnz and np.array_equal(ip, want[0]) and np.array_equal(self.csr[1], want[1])

    def forest(self, sort=True):
        m = max(self.n - 1, 1)
        u, v, w, info = np.full(m, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32), np.full(m, -7.0), np.full(3, -7, dtype=np.int64)
        self.e._check(self.L.as_graph_forest(self.e.sp, self.e.gr, int(sort), u.ctypes.data, v.ctypes.data, w.ctypes.data, info.ctypes.data))
        m = int(info[0])
        assert (u[m:] == -7).all() and (w[m:] == -7.0).all()   # nothing is written behind the edges
        return (u[:m], v[:m], w[:m]), dict(zip(("edges", "components", "rounds"), info.tolist()))

    def labels(self, t=None):
        return self.components(t)

    def tune(self, key, value):
        assert self.L.as_set_tuning(key, value) == 0


class Built:
    """A built shape behind the same three calls, through the Python methods."""

    def __init__(self, name):
        self.ix, self.csr = shape_csr(name)
        self.n = self.ix.n

    def forest(self, sort=True):
        return self.ix.aspace.spanning_forest(self.ix.gl, with_info=True, sort=sort)

    def labels(self, t=None):
        return self.ix.aspace.components(self.ix.gl, t, with_info=True)

    def tune(self, key, value):
        assert self.ix.asp._L.as_set_tuning(key, value) == 0


def case(name):
    if name not in _cases:
        _cases[name] = Built(name) if name in dfr.SHAPES else ForestHand(name)
        c = _cases[name]
        c.want = fr.kruskal(c.n, *c.csr)   # computed once, never written
    return _cases[name]


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:2], want[:2])) and np.array_equal(got[2].view(np.int64), want[2].view(np.int64))


def counters(ix):
    out = (C.c_int64 * 4)()
    assert ix.asp._L.as_forest_counters(ix.aspace._h, out, 4) == 0
    return list(out)


@pytest.mark.parametrize("name", HAND + list(dfr.SHAPES))
def test_the_edges_are_kruskals_in_the_total_order(name):
    c = case(name)
    if name == "twoway":   # or the case shows nothing: a pair whose two stored entries differ, one of them by a NaN
        ip, ci, dd = c.csr
        rows = np.repeat(np.arange(c.n), np.diff(ip))
        back = {(int(i), int(j)): d for i, j, d in zip(rows, ci, dd)}
        differ = [(i, j) for (i, j), d in back.items() if i < j and not np.isnan(d) and not np.isnan(back[j, i]) and d != back[j, i]]
        oneway_nan = [(i, j) for (i, j), d in back.items() if np.isnan(d) and not np.isnan(back[j, i])]
        assert len(differ) >= 32 and len(oneway_nan) == 1
    (u, v, w), info = c.forest()
    assert u.dtype == np.int32 and v.dtype == np.int32 and w.dtype == np.float64 and (u < v).all()
    assert same((u, v, w), c.want), name
    count = c.labels()[1]["count"]
    assert info["edges"] == len(u) == c.n - count and info["components"] == count
    print(f"{name}: n = {c.n}, {info['edges']} edges, {info['rounds']} rounds")
    assert 1 <= info["rounds"] <= math.ceil(math.log2(c.n)) + 1
    if name == "nan":
        assert int(np.isnan(w).sum()) == 2 and np.isnan(w[-2:]).all()   # two of the three NaN pairs join the three arcs, last
    if name == "monotone":
        assert len(u) == fr.MONOTONE_N - 1 and (np.diff(w) > 0).all()


@pytest.mark.parametrize("name", ["bridged", "path"] + list(dfr.SHAPES))
def test_cutting_the_forest_gives_the_components_at_every_threshold(name):
    c = case(name)
    (u, v, w), _ = c.forest()
    for t in cr.gap_thresholds(c.csr[2], 5) + [None]:
        labels, info = c.labels(t)
        assert np.array_equal(fr.cut(c.n, u, v, w, t), labels), t
        assert c.n - (len(w) if t is None else int((w <= t).sum())) == info["count"], t


@pytest.mark.parametrize("name", ["monotone", "hubs"] + list(dfr.SHAPES))
def test_determinism_over_repeats_grids_and_row_lanes(name):
    c = case(name)
    want, slots = c.forest()[0], c.forest(sort=False)[0]
    assert same(want, c.want)
    order = np.lexsort((slots[1], slots[0], np.where(np.isnan(slots[2]), np.inf, slots[2]), np.isnan(slots[2])))
    assert same(tuple(a[order] for a in slots), want)   # the slot order holds the same edges
    try:
        for cap, lanes in ((2, 0), (0, 8), (2, 32), (0, 0)):
            c.tune(b"diffuse_grid_cap", cap)
            c.tune(b"forest_row_lanes", lanes)
            for _ in range(2):
                assert same(c.forest()[0], want) and same(c.forest(sort=False)[0], slots), (cap, lanes)
    finally:
        c.tune(b"diffuse_grid_cap", 0)
        c.tune(b"forest_row_lanes", 0)


def test_two_host_threads_get_the_serial_answer():
    c = case("B")
    aspace, gl = c.ix.aspace, c.ix.gl
    labels, slots = aspace.components(gl), c.forest(sort=False)[0]
    errors = []

    def run(which):
        try:
            for _ in range(3):
                if which == 0:
                    assert same(aspace.spanning_forest(gl), c.want) and same(aspace.spanning_forest(gl, sort=False), slots)
                else:
                    assert same(aspace.spanning_forest(gl, sort=False), slots) and np.array_equal(aspace.components(gl), labels)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


def test_refusals_launch_nothing_and_leave_the_counters():
    ix, other = index("A"), index("B")
    L, EINVAL, EUNSUPPORTED = ix.asp._L, ix.asp._lib.AS_EINVAL, ix.asp._lib.AS_EUNSUPPORTED
    if "feature" not in _built:
        X = clustered(300, 12, nclust=6, seed=18)
        gp = {"eps": calibrate_feature_eps(X, 4), "k": 4, "topk": 8, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
              "lambda_mode": "feature"}
        _built["feature"] = Index(X, gp)
    fx = _built["feature"]
    before = [counters(x) for x in (ix, other, fx)]
    u, v, w = np.zeros(1000, dtype=np.int32), np.zeros(1000, dtype=np.int32), np.zeros(1000)
    with pytest.raises(ValueError, match="feature-mode"):
        fx.aspace.spanning_forest(fx.gl)
    assert L.as_graph_forest(fx.aspace._h, fx.gl._h, 1, u.ctypes.data, v.ctypes.data, w.ctypes.data, None) == EUNSUPPORTED
    for a, b in ((ix, other), (other, ix)):   # the graph of a space of another size, either way round
        with pytest.raises(ValueError):
            a.aspace.spanning_forest(b.gl)
        assert L.as_graph_forest(a.aspace._h, b.gl._h, 1, u.ctypes.data, v.ctypes.data, w.ctypes.data, None) == EINVAL
    for bad in (None, ix.aspace, "gl"):       # no graph at all
        with pytest.raises(TypeError):
            ix.aspace.spanning_forest(bad)
    assert L.as_graph_forest(ix.aspace._h, None, 1, u.ctypes.data, v.ctypes.data, w.ctypes.data, None) == EINVAL
    assert L.as_graph_forest(ix.aspace._h, ix.gl._h, 1, None, v.ctypes.data, w.ctypes.data, None) == EINVAL
    assert [counters(x) for x in (ix, other, fx)] == before
    # ... and a call that passes counts: one init, one weights launch, four per round, three of the emit; a wait per round and two
    (_, _, _), info = ix.aspace.spanning_forest(ix.gl, with_info=True)
    delta = [a - b for a, b in zip(counters(ix), before[0])]
    assert delta == [1, info["rounds"], 5 + 4 * info["rounds"], info["rounds"] + 2]
    assert ix.aspace.spanning_forest_counters() == dict(zip(("calls", "rounds", "launches", "host waits"), counters(ix)))
