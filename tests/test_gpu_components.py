"""GPU: connected components of the item graph -- ArrowSpace.components / components_sweep, GraphLaplacian.to_csr_dist and the C
entries behind them.  Every expected label and number comes from tests/components_ref.py (a union-find) on the CSR
the device itself stores, read through `as_graph_csr_dist`, so only the new code is under test; `rounds` depends on the schedule and
is only bounded.  Hand-built graphs go through `HipEngine.graph_from_knn` with the list helpers of tests/test_gpu_graph_stage.py and
call the C entries on the engine's handles; the built shapes A and B are the indices of tests/test_gpu_diffuse.py.
tests/test_components_inputs.py shows on the CPU the properties of the inputs the checks lean on."""
import ctypes as C
import threading

import numpy as np
import pytest

import components_ref as cr
import diffuse_ref as dfr
import test_gpu_graph_stage as gs
from conftest import calibrate_feature_eps, clustered
from oracle import oracle_np
from test_gpu_diffuse import Index, _built, index, tune

pytestmark = pytest.mark.gpu

NAMES = ("calls", "thresholds served", "hook launches", "compress launches", "host waits")
RING_SIZES = [1, 2, 63, 64, 65, 255, 256, 257]
PATH_N, PATH_SEED = 4099, 7
BRIDGED = (63, 70)
NAN_PAIRS = (10, 30, 50)     # "nan": the ring of 65 items (k = 1) whose pairs (i, i + 1) at these i carry a NaN dist
_engines = {}


# ------------------------------------------------------------------------------------------------ inputs (no GPU: the CPU file imports them)
def hand_case(name):
    """-> (X, graph parameters, lists) of a hand-built graph: a case of tests/test_gpu_graph_stage.py by its name, or one of
    "path" (the scrambled path), "bridged" (two rings and one bridge of the largest dist), "nan" (a ring with NaN dists)."""
    if name == "path":
        X = clustered(PATH_N, gs.D, nclust=6, seed=41)
        _, lists = gs.lists_from_neighbours(X, "l2", cr.path_lists(PATH_N, PATH_SEED))
        return X, gs.graph_params("l2", "gaussian", 2.0, 2, lists), lists
    if name == "bridged":
        nbrs, dists, _ = cr.bridged(*BRIDGED)
        X = clustered(sum(BRIDGED), gs.D, nclust=6, seed=42)
        _, lists = gs.lists_from_neighbours(X, "l2", nbrs)
        made = [dict(zip(js, ds)) for js, ds in zip(nbrs, dists)]
        lists = [(js, key, np.array([made[i][int(j)] for j in js], dtype=np.float64), gy) for i, (js, key, _, gy) in enumerate(lists)]
        return X, gs.graph_params("l2", "gaussian", 2.0, 2, lists), lists
    if name == "nan":
        X, gp, _, lists = gs.graph_case("ring65k1")
        lists = [(js, key, np.full_like(dd, np.nan) if i in NAN_PAIRS else dd, gy) for i, (js, key, dd, gy) in enumerate(lists)]
        return X, gp, lists
    X, gp, _, lists = gs.graph_case(name)
    return X, gp, lists


def sweep_thresholds(dist):
    """The 12 distinct thresholds of the sweep test: nine in gaps, a stored distance (kept: <=) and the two infinities."""
    return cr.gap_thresholds(dist, 9) + [float(np.sort(dist)[dist.shape[0] // 3]), np.inf, -np.inf]


def lists_csr(lists):
    """The CSR of components_ref.csr_of_lists for the lists of a hand case."""
    return cr.csr_of_lists(len(lists), [l[0].tolist() for l in lists], [l[2].tolist() for l in lists])


# ------------------------------------------------------------------------------------------------ GPU side
class Hand:
    """One engine per hand-built case for the whole module, with the CSR the device stores."""

    def __init__(self, name):
        X, gp, lists = hand_case(name)
        self.e = gs._engine(gp, X)
        self.e.graph_from_knn(*[gs._dev(a) for a in gs.pack_lists(lists, gp["k"])])
        self.L, self.n = self.e.L, X.shape[0]
        nnz = int(self.L.as_graph_nnz(self.e.gr)) - self.n
        ip, ix, dd = np.zeros(self.n + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64), np.zeros(max(nnz, 1))
        self.e._check(self.L.as_graph_csr_dist(self.e.gr, ip.ctypes.data, ix.ctypes.data, dd.ctypes.data))
        assert ip[self.n] == nnz
        self.csr = (ip, ix[:nnz], dd[:nnz])
        want = lists_csr(lists)   # the structure is the lists', both directions
        assert np.array_equal(ip, want[0]) and np.array_equal(self.csr[1], want[1])

    def components(self, t=None):
        labels, info = np.full(self.n, -7, dtype=np.int32), np.full(6, -7, dtype=np.int64)
        td = None if t is None else C.byref(C.c_double(t))
        self.e._check(self.L.as_graph_components(self.e.sp, self.e.gr, td, labels.ctypes.data, info.ctypes.data))
        return labels, dict(zip(cr.KEYS + ("rounds",), info.tolist()))

    def sweep(self, ts):
        ts = np.array(ts, dtype=np.float64)
        info = np.full((len(ts), 6), -7, dtype=np.int64)
        self.e._check(self.L.as_graph_components_sweep(self.e.sp, self.e.gr, ts.ctypes.data, len(ts), info.ctypes.data))
        return info

    def counters(self):
        out = (C.c_int64 * 5)()
        assert self.L.as_components_counters(self.e.sp, out, 5) == 0
        return list(out)

    def grid_cap(self, cap):
        assert self.L.as_set_tuning(b"diffuse_grid_cap", cap) == 0


def hand(name):
    if name not in _engines:
        _engines[name] = Hand(name)
    return _engines[name]


def check(n, csr, got, t, what):
    """Labels and info of one call against the union-find on `csr`; -> (labels, info)."""
    labels, info = got
    want = cr.components(n, *csr, t)
    assert labels.dtype == np.int32 and labels.shape == (n,), what
    assert np.array_equal(labels, want), what
    assert {k: info[k] for k in cr.KEYS} == cr.info(want, *csr, t), what
    assert info["rounds"] >= 1, what
    return labels, info


def check_hand(name, thresholds=(None,)):
    h = hand(name)
    return h, [check(h.n, h.csr, h.components(t), t, (name, t)) for t in thresholds]


def index_counters(ix):
    out = (C.c_int64 * 5)()
    assert ix.asp._L.as_components_counters(ix.aspace._h, out, 5) == 0
    return list(out)


def shape_csr(name):
    ix = index(name)
    if not hasattr(ix, "csr_dist"):
        ix.csr_dist = ix.gl.to_csr_dist()
    return ix, ix.csr_dist


# ------------------------------------------------------------------------------------------------ A. hand-built graphs
def test_the_scrambled_path_ends_within_the_round_cap():
    h, ((labels, info),) = check_hand("path")
    assert (labels == 0).all() and info["count"] == 1 and info["largest"] == PATH_N and info["edges_kept"] == 2 * (PATH_N - 1)
    print(f"scrambled path of {PATH_N}: {info['rounds']} rounds (the synchronous reference lowers in 8)")
    assert info["rounds"] <= cr.ROUND_CAP
    try:
        h.grid_cap(2)   # two blocks take the 17 row groups in grid-stride trips
        capped, cinfo = check(h.n, h.csr, h.components(), None, "path, grid cap 2")
        assert np.array_equal(capped, labels) and cinfo["rounds"] <= cr.ROUND_CAP
    finally:
        h.grid_cap(0)


def test_hubs_rows_of_thousands_of_entries_and_rows_without_one():
    h, ((labels, info),) = check_hand("hubs")
    deg = np.diff(h.csr[0])
    assert h.n == 4100 and deg.max() >= 2000 and (deg == 0).any()
    assert info["isolated"] == int((deg == 0).sum()) and info["count"] > 1
    d = h.csr[2]
    for t in cr.gap_thresholds(d, 3) + [float(np.median(d))]:
        check(h.n, h.csr, h.components(t), t, ("hubs", t))


def test_a_graph_without_an_edge():
    h, ((labels, info),) = check_hand("empty")
    assert h.n == 1025 and np.array_equal(labels, np.arange(1025))
    assert info == {"count": 1025, "largest": 1, "largest_label": 0, "isolated": 1025, "edges_kept": 0, "rounds": 1}
    labels, info = check(h.n, h.csr, h.components(1.0), 1.0, "empty, a threshold")
    assert info["rounds"] == 1 and info["count"] == 1025


@pytest.mark.parametrize("n", RING_SIZES)
def test_rings_at_wave_and_block_edges(n):
    for k in (1, 3):
        h, ((labels, info),) = check_hand("ring%dk%d" % (n, k))
        assert (labels == 0).all() and info["count"] == 1 and info["largest"] == n and info["isolated"] == (1 if n == 1 else 0)


@pytest.mark.parametrize("name", ["duplicates", "wide"])
def test_duplicates_and_wide_lists(name):
    h, ((labels, info),) = check_hand(name)
    if name == "duplicates":   # 0 and 1 list only each other; 2 .. 5 hang on the ring of 8 .. 63; 6 and 7 list nothing
        assert labels[:8].tolist() == [0, 0, 2, 2, 2, 2, 6, 7] and (labels[8:] == 2).all()
        assert info["count"] == 4 and info["isolated"] == 2
    d = h.csr[2]
    for t in cr.gap_thresholds(d, 3) + [0.0]:   # (the duplicates' pairs have dist 0: kept at t = 0)
        check(h.n, h.csr, h.components(t), t, (name, t))


def test_the_bridge_joins_two_rings_at_its_own_distance_and_not_below():
    h = hand("bridged")
    n_a, n_b = BRIDGED
    d = h.csr[2]
    bridge = float(d.max())
    assert bridge == 2.0 and int((d == bridge).sum()) == 2 and np.sort(d)[-3] < 1.5   # the pair's two entries, strictly the largest
    below = 0.5 * (np.sort(d)[-3] + bridge)
    for t, count in ((None, 1), (bridge, 1), (below, 2)):
        labels, info = check(h.n, h.csr, h.components(t), t, ("bridged", t))
        assert info["count"] == count
        assert set(labels.tolist()) == ({0} if count == 1 else {0, n_a})
        if count == 2:
            assert (labels[:n_a] == 0).all() and (labels[n_a:] == n_a).all()
            assert info["largest"] == n_b and info["largest_label"] == n_a and info["edges_kept"] == 2 * (n_a + n_b)


def test_thresholds_at_the_infinities_at_a_stored_distance_and_nan_distances():
    h = hand("hubs")
    d = h.csr[2]
    assert np.isfinite(d).all()
    labels, info = check(h.n, h.csr, h.components(-np.inf), -np.inf, "-inf")
    assert np.array_equal(labels, np.arange(h.n)) and info["edges_kept"] == 0 and info["rounds"] == 1
    all_labels, all_info = h.components()
    labels, info = check(h.n, h.csr, h.components(np.inf), np.inf, "+inf")
    assert np.array_equal(labels, all_labels) and info["edges_kept"] == all_info["edges_kept"] == d.shape[0]
    # a threshold equal to a stored distance keeps that entry; the next double below drops it
    at = float(np.sort(d)[d.shape[0] // 2])
    _, i_at = check(h.n, h.csr, h.components(at), at, "at a stored distance")
    lower = float(np.nextafter(at, -np.inf))
    _, i_lo = check(h.n, h.csr, h.components(lower), lower, "one ulp below")
    assert i_at["edges_kept"] - i_lo["edges_kept"] == int((d == at).sum()) >= 1
    # NaN distances: kept only without a threshold
    h = hand("nan")
    d = h.csr[2]
    assert int(np.isnan(d).sum()) == 2 * len(NAN_PAIRS)
    labels, info = check(h.n, h.csr, h.components(), None, "nan, no threshold")
    assert (labels == 0).all() and info["edges_kept"] == d.shape[0]
    labels, info = check(h.n, h.csr, h.components(np.inf), np.inf, "nan, +inf")
    assert info["count"] == len(NAN_PAIRS) and info["edges_kept"] == d.shape[0] - 2 * len(NAN_PAIRS)
    assert sorted(set(labels.tolist())) == [0] + [i + 1 for i in NAN_PAIRS[:-1]]   # the arcs between the cut pairs (the last wraps to 0)
    nan = C.c_double(float("nan"))
    c0 = h.counters()
    assert h.L.as_graph_components(h.e.sp, h.e.gr, C.byref(nan), labels.ctypes.data, None) == h.e._lib.AS_EINVAL
    assert "NaN" in h.e._lib.last_error() and h.counters() == c0


# ------------------------------------------------------------------------------------------------ B. the built shapes
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_to_csr_dist_against_to_csr_and_the_oracle(name):
    ix, (ip, ci, dd) = shape_csr(name)
    assert ip.dtype == np.int64 and ci.dtype == np.int64 and dd.dtype == np.float64
    assert np.array_equal(ip, ix.op[0]) and np.array_equal(ci, ix.op[1])   # to_csr() with its diagonal removed
    metric = oracle_np.METRIC_L2 if ix.gp["metric"] == "l2" else oracle_np.METRIC_COSINE
    n64 = np.einsum("ij,ij->i", ix.X, ix.X)
    worst = 0.0
    for i in range(ix.n):
        js = ci[ip[i]:ip[i + 1]]
        if len(js):
            want = oracle_np.pair_quantities(ix.X[i], ix.X[js], n64[i], n64[js], metric)[1]
            worst = max(worst, gs._reldiff(dd[ip[i]:ip[i + 1]], want))
    print(f"{name}: to_csr_dist against oracle_np.pair_quantities: {worst:.3g} relative at most")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_built_shapes_without_a_threshold_and_at_five_thresholds(name):
    ix, csr = shape_csr(name)
    labels, info = check(ix.n, csr, ix.aspace.components(ix.gl, with_info=True), None, (name, None))
    assert info["count"] > 1 and info["isolated"] >= 1
    assert isinstance(info, dict) and list(info) == list(cr.KEYS) + ["rounds"] and all(type(v) is int for v in info.values())
    plain = ix.aspace.components(ix.gl)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, labels)
    for t in cr.gap_thresholds(csr[2], 5):
        assert cr.gap_of(csr[2], t) > 0.0
        check(ix.n, csr, ix.aspace.components(ix.gl, t, with_info=True), t, (name, t))


# ------------------------------------------------------------------------------------------------ C. sweep, determinism, ties, refusals, threads
@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_a_sweep_equals_the_loop_of_single_calls(name):
    ix, csr = shape_csr(name)
    base = sweep_thresholds(csr[2])
    ts = [base[i] for i in np.random.default_rng(3).permutation(len(base))] + [base[2], base[2], base[7], np.inf]   # 16, shuffled, duplicates
    assert len(ts) == 16 and len(set(ts)) == 12
    singles = [ix.aspace.components(ix.gl, t, with_info=True)[1] for t in ts]
    c0 = index_counters(ix)
    got = ix.aspace.components_sweep(ix.gl, ts)
    c1 = index_counters(ix)
    assert list(got) == list(cr.KEYS) + ["rounds"]
    for k in cr.KEYS:
        assert got[k].dtype == np.int64 and got[k].tolist() == [s[k] for s in singles], k
    assert (got["rounds"] >= 1).all()
    # one call, 16 thresholds served by the stages of the 12 distinct ones: a duplicate reports its stage's rounds and launches nothing
    first = {t: i for i, t in reversed(list(enumerate(ts)))}
    rounds = sum(int(got["rounds"][i]) for i in first.values())
    assert all(got["rounds"][i] == got["rounds"][first[t]] for i, t in enumerate(ts))
    assert [a - b for a, b in zip(c1, c0)] == [1, 16, rounds, rounds, rounds + 12]
    assert ix.aspace.components_counters() == dict(zip(NAMES, c1))
    print(f"{name}: the sweep's 12 stages ran {rounds} rounds, the 12 cold single calls {sum(singles[i]['rounds'] for i in first.values())}")


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_determinism_over_repeats_and_grids(name):
    ix, csr = shape_csr(name)
    t = cr.gap_thresholds(csr[2], 5)[3]
    strip = lambda info: {k: info[k] for k in cr.KEYS}   # noqa: E731
    try:
        want = [ix.aspace.components(ix.gl, th, with_info=True) for th in (None, t)]
        for cap in (0, 2, 0):
            tune(ix, {b"diffuse_grid_cap": cap})
            for th, (labels, info) in zip((None, t), want):
                again, ainfo = ix.aspace.components(ix.gl, th, with_info=True)
                assert np.array_equal(again, labels) and strip(ainfo) == strip(info), (cap, th)
    finally:
        tune(ix, {})


def test_ties_to_diffusion_grouped_search_and_subsets():
    ix, csr = shape_csr("B")
    aspace, gl = ix.aspace, ix.gl
    labels, info = aspace.components(gl, with_info=True)
    # diffusion never leaves the seed's component
    for s in (info["largest_label"], int(np.flatnonzero(labels != info["largest_label"])[0])):
        f = aspace.diffuse(gl, [([s], [1.0])], 0.5, 7)[0]
        assert (f[labels != labels[s]] == 0.0).all() and f[s] != 0.0
    # the labels are group labels: every returned group holds items of one component
    groups = aspace.groups(labels)
    for q in ix.queries(np.random.default_rng(5), 3):
        answer = aspace.search_grouped(q, gl, dfr.TAU, groups, 4, 3)
        assert len(answer) >= 1
        for label, members in answer:
            assert len(members) >= 1 and all(labels[i] == label for i, _ in members)
    assert aspace.subset(labels == info["largest_label"]).size == info["largest"]


def test_refusals_launch_nothing_and_leave_the_counters():
    ix, other = index("A"), index("B")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    L, EINVAL, EUNSUPPORTED = asp._L, asp._lib.AS_EINVAL, asp._lib.AS_EUNSUPPORTED
    labels, info = np.zeros(1000, dtype=np.int32), np.zeros((65, 6), dtype=np.int64)
    ts = np.linspace(0.1, 1.0, 65)
    c0, o0 = index_counters(ix), index_counters(other)
    # a NaN threshold, T out of range
    for call in (lambda: aspace.components(gl, float("nan")), lambda: aspace.components_sweep(gl, [0.5, float("nan")]),
                 lambda: aspace.components_sweep(gl, []), lambda: aspace.components_sweep(gl, ts), lambda: aspace.components(gl, "0.5")):
        with pytest.raises(ValueError):
            call()
    bad = np.array([0.5, np.nan])
    assert L.as_graph_components_sweep(aspace._h, gl._h, bad.ctypes.data, 2, info.ctypes.data) == EINVAL and "NaN" in asp._lib.last_error()
    for nt in (0, 65, -1):
        assert L.as_graph_components_sweep(aspace._h, gl._h, ts.ctypes.data, nt, info.ctypes.data) == EINVAL
        assert "[1, 64]" in asp._lib.last_error()
    assert L.as_graph_components(aspace._h, gl._h, None, None, info.ctypes.data) == EINVAL
    # the graph of a space of another size, either way round
    with pytest.raises(ValueError):
        aspace.components(other.gl)
    with pytest.raises(ValueError):
        other.aspace.components_sweep(gl, [0.5])
    assert L.as_graph_components(aspace._h, other.gl._h, None, labels.ctypes.data, None) == EINVAL
    # a feature-mode index
    if "feature" not in _built:
        X = clustered(300, 12, nclust=6, seed=18)
        gp = {"eps": calibrate_feature_eps(X, 4), "k": 4, "topk": 8, "p": 2.0, "sigma": None, "metric": "cosine", "kernel": "rational",
              "lambda_mode": "feature"}
        _built["feature"] = Index(X, gp)
    fx = _built["feature"]
    f0 = index_counters(fx)
    assert L.as_graph_components(fx.aspace._h, fx.gl._h, None, labels.ctypes.data, None) == EUNSUPPORTED
    assert L.as_graph_components_sweep(fx.aspace._h, fx.gl._h, ts.ctypes.data, 3, info.ctypes.data) == EUNSUPPORTED
    for call in (lambda: fx.aspace.components(fx.gl), lambda: fx.aspace.components_sweep(fx.gl, [0.5]), lambda: fx.gl.to_csr_dist()):
        with pytest.raises(ValueError, match="feature-mode"):
            call()
    assert index_counters(fx) == f0 and index_counters(ix) == c0 and index_counters(other) == o0


def test_two_host_threads_get_the_serial_answers():
    ix, csr = shape_csr("B")
    aspace, gl = ix.aspace, ix.gl
    Q = ix.queries(np.random.default_rng(31), 6)
    ts = [None] + cr.gap_thresholds(csr[2], 3)
    strip = lambda got: (got[0].tolist(), {k: got[1][k] for k in cr.KEYS})   # noqa: E731
    serial_c = [strip(aspace.components(gl, t, with_info=True)) for t in ts]
    serial_d = [aspace.search_diffuse(q, gl, dfr.TAU, 0.85, 5) for q in Q]
    errors = []

    def run(which):
        try:
            for _ in range(3):
                if which == 0:
                    assert [strip(aspace.components(gl, t, with_info=True)) for t in ts] == serial_c
                else:
                    assert [aspace.search_diffuse(q, gl, dfr.TAU, 0.85, 5) for q in Q] == serial_d
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
