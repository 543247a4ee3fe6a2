"""GPU: shortest paths over the item graph -- ArrowSpace.shortest_paths / score_geodesic / search_geodesic / search_batch_geodesic
and the C entries behind them.  Every expected distance comes from tests/geodesic_ref.py (a heap Dijkstra with
Python float adds) on the CSR the device itself stores, and every comparison is of bits: the least fixed point is unique, so no
tolerance is needed.  The hand-built graphs are those of tests/test_gpu_forest.py; the built shapes are test_gpu_diffuse.py's."""
import ctypes as C

import numpy as np
import pytest

import diffuse_ref as dfr
import geodesic_ref as gr
from test_gpu_components import RING_SIZES, shape_csr
from test_gpu_diffuse import TAU, Index, batch_pools
from test_gpu_forest import ForestHand

pytestmark = pytest.mark.gpu

HAND = (["path", "hubs", "empty"] + ["ring%dk%d" % (n, k) for n in RING_SIZES for k in (1, 2)]
        + ["duplicates", "wide", "bridged", "nan", "twoway", "monotone"])
TUNINGS = (b"diffuse_cols", b"diffuse_grid_cap", b"geodesic_row_lanes")
_cases = {}


class Case:
    """A hand-built graph (the C entries on the engine's handles) or a built shape (the index's), with the CSR the device stores,
    its undirected weights and the Dijkstra of every source set asked for so far (computed once, never written)."""

    def __init__(self, name):
        import pyarrowspace_amd as asp
        self.asp, self.L = asp, asp._L
        if name in dfr.SHAPES:
            self.ix, self.csr = shape_csr(name)
            self.n, self.sp, self.gr = self.ix.n, self.ix.aspace._h, self.ix.gl._h
        else:
            self.hand = ForestHand(name)
            self.n, self.csr, self.sp, self.gr = self.hand.n, self.hand.csr, self.hand.e.sp, self.hand.e.gr
        self.w = gr.weights(self.n, *self.csr)
        self._ref = {}

    def ref(self, source):
        ids, offs = ([source], [0.0]) if isinstance(source, int) else source
        key = (tuple(ids), tuple(offs))
        if key not in self._ref:
            self._ref[key] = gr.dijkstra(self.n, self.csr[0], self.csr[1], self.w, ids, offs)
        return self._ref[key]

    def want(self, sources, cutoff=None):
        d = np.stack([self.ref(s) for s in sources]) if len(sources) else np.empty((0, self.n))
        return d if cutoff is None else np.where(d <= cutoff, d, np.inf)

    def paths(self, sources, cutoff=None, pick=None):
        """as_geodesic_seeds -> (d, info)"""
        ids, offs, starts = self.asp.ArrowSpace._geodesic_sources(sources, self.n)
        b, m = len(sources), self.n if pick is None else len(pick)
        out, info = np.full((b, m), -7.0), np.zeros(2 + 2 * b, dtype=np.int64)
        pick = None if pick is None else np.asarray(pick, dtype=np.int64)
        rc = self.L.as_geodesic_seeds(self.sp, self.gr, ids.ctypes.data, offs.ctypes.data, starts.ctypes.data, b,
                                      None if cutoff is None else C.byref(C.c_double(cutoff)), None if pick is None else pick.ctypes.data, m,
                                      out.ctypes.data, info.ctypes.data)
        assert rc == 0, self.asp._lib.last_error()
        return out, info

    def tune(self, setting, delta=0.0, lds_rows=-1):
        for key in TUNINGS:
            assert self.L.as_set_tuning(key, setting.get(key, 0)) == 0
        assert self.L.as_set_tuning(b"geodesic_lds_rows", lds_rows) == 0
        self.L.as_set_geodesic_delta(delta)

    def sources(self):
        """An item, a set with unequal offsets (one a -0.0), the empty set, the last item."""
        some = sorted({1 % self.n, self.n // 2, self.n - 1})
        return [0, (some, [0.25, -0.0, 1.5][:len(some)]), ([], []), self.n - 1]


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", HAND + list(dfr.SHAPES))
def test_distances_are_dijkstras_by_the_push_and_the_pull_route(name):
    c = case(name)
    src = c.sources()
    want = c.want(src)
    assert np.isinf(want[2]).all() and want[0, 0] == 0.0 and not np.signbit(want[1]).any()
    if name == "empty":
        assert np.isfinite(want).sum() == 1 + len(src[1][0]) + 1   # the sources' own entries alone
    try:
        for cols in (1, 0):   # every column on its own by the frontier; one chunk of 16 columns
            c.tune({b"diffuse_cols": cols})
            d, info = c.paths(src)
            assert same(d, want), (name, cols)
            assert info[0] == (len(src) if cols else 1) and info[2 + len(src):].tolist() == np.isfinite(want).sum(axis=1).tolist()
            print(f"{name}: n = {c.n}, cols {cols}: rounds {info[2:2 + info[0]].tolist()}, {info[1]} relaxations")
    finally:
        c.tune({})


@pytest.mark.parametrize("b", [1, 2, 16, 17, 64, 65])
def test_source_counts_across_the_column_widths_and_a_second_chunk(b):
    c = case("B")
    src = [int(i) for i in np.random.default_rng(5).choice(c.n, 65, replace=False)][:b]
    want = c.want(src)
    try:
        for cols in (0, 1, 16, 64) if b == 65 else (0,):
            c.tune({b"diffuse_cols": cols})
            d, info = c.paths(src)
            assert same(d, want), (b, cols)
            chunks = {0: {1: 1, 2: 1, 16: 1, 17: 2, 64: 1, 65: 2}[b], 1: b, 16: 5, 64: 2}[cols]
            assert info[0] == chunks, (b, cols)
    finally:
        c.tune({})


def _deltas(c):
    pos = np.sort(c.w[c.w > 0.0])
    return [float(pos[0]), float(pos[len(pos) // 2]), 1e300]


SETTINGS = ([({b"diffuse_grid_cap": cap}, None, -1) for cap in (1, 3)] + [({b"geodesic_row_lanes": lanes}, None, -1) for lanes in (8, 32)]
            + [({}, which, -1) for which in (0, 1, 2)] + [({}, None, 0), ({}, None, 64), ({b"diffuse_grid_cap": 3, b"geodesic_row_lanes": 8}, 1, 64)])


@pytest.mark.parametrize("setting,which_delta,lds_rows", SETTINGS)
@pytest.mark.parametrize("name", ["path", "hubs", "duplicates", "B"])
def test_the_same_bits_under_every_tuning(name, setting, which_delta, lds_rows):
    c = case(name)
    src = c.sources()[:2]
    want = c.want(src)
    delta = 0.0 if which_delta is None else _deltas(c)[which_delta]
    try:
        c.tune({**setting, b"diffuse_cols": 1}, delta, lds_rows)
        d, info = c.paths(src)
        assert same(d, want), "push"
        if lds_rows == 64 and which_delta is None and name in ("hubs", "B"):   # one bucket: the frontier outgrew the LDS lists and spilled
            assert c.L.as_geodesic_kernel_us(c.sp, 9) >= 1 and c.L.as_geodesic_kernel_us(c.sp, 10) >= 1
        if lds_rows == 0:
            assert c.L.as_geodesic_kernel_us(c.sp, 9) == 0
        c.tune(setting, delta, lds_rows)
        assert same(c.paths(src)[0], want), "pull"
    finally:
        c.tune({})


@pytest.mark.parametrize("name", ["hubs", "bridged", "monotone", "B"])
def test_a_cutoff_keeps_the_bits_inside_the_ball_and_nothing_outside(name):
    c = case(name)
    src = c.sources()
    full = c.want(src)
    try:
        for cols in (1, 0):
            c.tune({b"diffuse_cols": cols})
            for cutoff in (0.0, float(np.median(full[np.isfinite(full)])), np.inf):
                d, info = c.paths(src, cutoff)
                assert same(d, c.want(src, cutoff)), (name, cols, cutoff)
        d, _ = c.paths([([0], [1.0])], 0.5)   # a source whose own offset lies above the cutoff
        assert np.isinf(d).all()
    finally:
        c.tune({})


@pytest.mark.parametrize("name", ["nan", "bridged", "A", "B"])
def test_finite_exactly_inside_the_sources_component(name):
    c = case(name)
    comp = (lambda t: c.ix.aspace.components(c.ix.gl, t)) if name in dfr.SHAPES else (lambda t: c.hand.components(t)[0])
    labels, numbered = comp(None), comp(np.inf)   # every stored entry; every entry whose dist is no NaN: the edges the paths cross
    src = [0, c.n // 3, c.n - 1]
    d, _ = c.paths(src)
    assert all(np.array_equal(np.isfinite(row), numbered == numbered[s]) for row, s in zip(d, src))
    if name == "nan":   # `components` without a threshold joins across the NaN pairs too: three arcs, one label
        assert len(np.unique(labels)) == 1 and len(np.unique(numbered)) == 3
    else:
        assert np.array_equal(labels, numbered)


def test_the_kept_weights_follow_the_graph_of_the_call():
    """Two graphs over the items of one space, alternating, and the hand-over from `spanning_forest`: every call reads its own
    graph's weights, whichever graph's images the workspace held before."""
    c = case("B")
    aspace, gl = c.ix.aspace, c.ix.gl
    other = Index(c.ix.X, dict(c.ix.gp, k=c.ix.gp["k"] // 2))   # the same items, half the neighbours: another CSR, other weights
    csr2 = other.gl.to_csr_dist()
    w2 = gr.weights(c.n, *csr2)
    src = [3, c.n // 2]
    want1 = c.want(src)
    want2 = np.stack([gr.dijkstra(c.n, csr2[0], csr2[1], w2, [s], [0.0]) for s in src])
    assert not same(want1, want2)
    for cols in (1, 0):
        c.tune({b"diffuse_cols": cols})
        try:
            for _ in range(2):
                assert same(aspace.shortest_paths(gl, src), want1) and same(aspace.shortest_paths(other.gl, src), want2)
            aspace.spanning_forest(other.gl)
            assert same(aspace.shortest_paths(other.gl, src), want2) and same(aspace.shortest_paths(gl, src), want1)
            aspace.spanning_forest(other.gl)
            assert same(aspace.shortest_paths(gl, src), want1) and same(aspace.shortest_paths(other.gl, src), want2)
        finally:
            c.tune({})


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_the_score_and_search_forms_against_the_composition(name):
    c = case(name)
    ix, aspace, gl = c.ix, c.ix.aspace, c.ix.gl
    rng = np.random.default_rng(11)
    src, pick = c.sources(), rng.integers(0, c.n, 37)
    assert same(aspace.score_geodesic(gl, src, pick), c.want(src)[:, pick])
    assert same(aspace.shortest_paths(gl, src), c.want(src))
    topk, ids = ix.topk(), np.sort(rng.choice(c.n, c.n // 3, replace=False))
    Q = np.stack(ix.queries(rng, 18) + [np.full(ix.d, 50.0)])   # the last: no item within eps, lambda_q == 0
    cutoff = float(np.median(c.w[c.w >= 0.0])) * 3
    for sub_ids in (None, ids):
        sub = None if sub_ids is None else aspace.subset(sub_ids)
        pools, status = batch_pools(ix, Q, TAU, sub)
        assert status[-1] == ix.asp._lib.AS_EZEROLAMBDA and not any(status[:-1])
        for seeds, cut in ((1, None), (topk, None), (2, cutoff)):
            want = [gr.search(c.n, c.csr[0], c.csr[1], c.w, p, seeds, topk, sub_ids, cut) if p else [] for p in pools]
            got = aspace.search_batch_geodesic(Q, gl, TAU, seeds, cut, sub)
            for g, w in zip(got, want):
                assert [i for i, _ in g] == [i for i, _ in w]
                assert same(np.array([v for _, v in g]), np.array([v for _, v in w]))
            assert got[-1] == [] and all(len(g) >= 1 for g in got[:-1])
            for q, p in list(zip(Q, want))[:3]:
                assert aspace.search_geodesic(q, gl, TAU, seeds, cut, sub) == p
    with pytest.raises(ix.asp.PanicException):
        aspace.search_geodesic(Q[-1], gl, TAU)
    before = aspace.geodesic_counters()
    aspace.search_geodesic(Q[0], gl, TAU)
    after = aspace.geodesic_counters()
    assert after["calls"] == before["calls"] + 1 and after["route searches"] == before["route searches"] + 1
    assert after["column chunks"] == before["column chunks"] + 1 and after["rounds"] > before["rounds"]
