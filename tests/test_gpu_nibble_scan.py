"""GPU: the single query's coarse scan on the NIBBLE tiles (scan_tile_kernel_dyn<.., NIB>, space_nib_image) against
the same searches on the 8-bit tiles -- hits, scores and lambda_q bit for bit -- and against the fp64 oracle (rtol 1e-9).

Data (make_data): clustered unit rows, 16 centres, noise 0.3 (conftest.clustered): the cosine is about 0.92 inside a cluster and
|cos| < 0.2 across clusters.  The nibble scan is priced with a coefficient of up to 0.17, so its scorer window reaches
W + 2 * 0.17 below the cosine bound, W = (1 - tau) / (2 tau): the input builder measures in fp64 whether that window stays clear
of the other clusters (`clear`: the smallest cosine to the Ms = 64 nearest rows' bin edge, minus the window, above the largest
cosine to another cluster) and ASSERTS it at tau = 0.62 and 1 for every index of 4 096 rows and more.  Where the window is clear
the search must be served by the nibble tiles without a rerun: last_scan_bits == 4, nibble_reruns unchanged.  At tau = 0.4
W = 0.75: the window takes in every row whatever the data, the candidates may or may not fit, and the route is outcome-driven --
there the test accepts either a clean nibble search or one rerun on 8 bits (nibble_reruns + 1, last_scan_bits == 8), and the
answer must be the same bits either way.  The same holds for the query with no row inside eps: a fresh direction has every
row at a cosine near zero, inside any window.  Those searches come LAST on their index: a rerun sends the workspace's next 63
searches past the tiles (where they were first run, the only reruns were the fresh direction's at 4 133 rows).  Every such
search must TRY the tiles (nibble_scans + 1) unless a rerun was already seen on its workspace.  At 100 rows a cluster has six
rows: no window is clear, all 100 rows are candidates of both widths, and they fit -- there every search at tau >= 0.4, the fresh
direction's included, must read 4 bits without a rerun.

Shapes, the smallest at which the kernel can go wrong: D = 512 (C4 = 16 chunks, the minimum of the ticket argument), 544
(dp8 = 576, C4 = 18: zero-padded columns), 768; N = 100 (fewer chunks than waves: tickets run past the end), 4 096 (whole
chunks), 4 133 (a partial last chunk); metrics l2 and cosine.  The scan runs with as_set_tuning("coarse_bits", 4): the route at any
row count, on the dynamic schedule.

Queries: a perturbed item, a fresh draw around a centre, a normalised cluster mean with more than 64 rows inside eps (asserted
in fp64; 4 096 rows and more), a fresh direction with no row inside eps (the zero-lambda panic: the same exception at both
widths, counted).  tau 0.62, 1.0, 0.4, and 0.2 -- the coarse chain, which must not take the nibble tiles."""
import functools

import numpy as np
import pytest

from conftest import assert_hits_match, calibrate_eps, clustered   # (calibrate_eps: the isotropic index)

pytestmark = pytest.mark.gpu

RTOL = 1e-9
NCLUST = 16
NOISE = 0.3
K = 40
TOPK = 8
MS = 64                 # the scorer's list: topk + margin rounded up to 64 (query_alloc)
COEF4 = 0.17            # what the nibble scan is priced with on such rows, at most (tools/nibble_sim.py; asserted on the GPU below)
ERR4 = 0.03             # the largest ACTUAL error of a coarse cosine on such rows (tools/nibble_sim.py: 0.029 over 64 000 pairs)
SHAPES = [(100, 512, "l2"), (4096, 512, "l2"), (4133, 512, "cosine"), (100, 544, "cosine"), (4096, 544, "l2"), (4133, 544, "l2"),
          (100, 768, "l2"), (4096, 768, "cosine"), (4133, 768, "l2")]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _window_clear(X, q, tau):
    """fp64: does (lower edge of the bin of the MS-th largest cosine) - W - 2 COEF4 lie above every cosine that is itself below
    the gap -- i.e. does the window end inside the gap between the query's cluster and the rest?"""
    c = np.sort((X @ q) / (np.linalg.norm(X, axis=1) * np.linalg.norm(q)))[::-1]
    if len(c) < MS:
        return False
    bound = np.floor((c[MS - 1] + 1.0) * 32.0) / 32.0 - 1.0
    low = bound - (1.0 - tau) / (2.0 * tau) - 2.0 * COEF4
    rest = c[c < 0.5]            # (the other clusters: cosines of 0.2 at most, asserted by make_data)
    return bool(len(rest) == 0 or low > rest.max() + ERR4)    # (+ what a coarse cosine is actually off by)


@functools.lru_cache(maxsize=None)
def make_data(n, d, metric):
    X = np.ascontiguousarray(clustered(n, d, nclust=NCLUST, noise=NOISE, seed=n + d))
    rng = np.random.default_rng(7 * n + d)
    G = X[: min(n, 512)] @ X.T
    assert ((G > 0.8) | (np.abs(G) < 0.2)).all()          # the recipe's margin: a cluster at cosine ~0.92, nothing between
    # eps: the 30 % quantile of the distances inside a cluster (the rows are unit: |x - y|^2 = 2 - 2 cos)
    within = G[(G > 0.8) & (G < 1.0 - 1e-9)]
    eps = float(np.quantile(np.sqrt(2.0 - 2.0 * within) if metric == "l2" else 1.0 - within, 0.3))
    gp = {"eps": eps, "k": K, "topk": TOPK, "p": 2.0, "sigma": None, "metric": metric}
    qs = {"perturbed": _unit(X[n // 3] + 0.02 * rng.standard_normal(d) / np.sqrt(d))}
    own = (X @ X[0]) > 0.8             # (row 0's cluster: its mean is the centre's direction)
    centre = _unit(X[own].mean(axis=0))
    qs["draw"] = _unit(centre * np.sqrt(d) + NOISE * rng.standard_normal(d))   # (the recipe: a centre of norm ~ sqrt(d), plus noise)
    qs["dense"] = centre
    qs["empty"] = _unit(rng.standard_normal(d))
    inside = {}
    for name, q in qs.items():
        cos = (X @ q) / np.linalg.norm(X, axis=1)
        dist = np.sqrt(np.maximum(1.0 + (X * X).sum(1) - 2.0 * (X @ q), 0.0)) if metric == "l2" else 1.0 - np.maximum(0.0, cos)
        inside[name] = int((dist <= gp["eps"]).sum())
    assert inside["empty"] == 0 and inside["perturbed"] > 0
    if n >= 4096:
        assert inside["dense"] > 64, inside
        for name in ("perturbed", "draw", "dense"):
            assert _window_clear(X, qs[name], 0.62) and _window_clear(X, qs[name], 1.0), name
    X.setflags(write=False)
    return X, gp, qs, inside


def _set_bits(v):
    import pyarrowspace_amd as asp
    assert asp._L.as_set_tuning(b"coarse_bits", v) == 0


@pytest.fixture(autouse=True)
def _restore_switch():
    try:
        yield
    finally:
        _set_bits(-1)


def _search(aspace, gl, q, tau, bits):
    """(hits or None for the zero-lambda panic, lambda_q, last_scan_bits, last_scan_operand, counters before, after)"""
    import pyarrowspace_amd as asp
    _set_bits(bits)
    c0 = aspace.search_counters()
    try:
        hits = aspace.search(q, gl, tau)
    except asp.PanicException:
        hits = None
    got_bits, op = aspace.last_scan_bits, aspace.last_scan_operand
    c1 = aspace.search_counters()
    return hits, aspace.query_lambda(q, gl), got_bits, op, c0, c1


@pytest.mark.parametrize("n,d,metric", SHAPES)
def test_nibble_scan_matches_8_bits_and_oracle(oracle_lib, n, d, metric):
    import pyarrowspace_amd as asp
    X, gp, qs, inside = make_data(n, d, metric)
    a4, g4 = asp.ArrowSpaceBuilder.build(gp, X)     # (a workspace per width: a rerun's skip count must not leak into the other)
    a8, g8 = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    # (the searches whose window is clear first, the outcome-driven ones behind them: see the module's docstring)
    cases = [(tau, name) for tau in (0.62, 1.0) for name in ("perturbed", "draw", "dense")]
    cases += [(tau, "empty") for tau in (0.62, 1.0)] + [(tau, name) for tau in (0.2, 0.4) for name in ("perturbed", "draw", "dense", "empty")]
    armed = False    # a nibble search of this workspace has ended in a rerun: its next 63 eligible searches may skip the tiles
    for tau, name in cases:
        q = qs[name]
        h4, l4, b4, op4, c0, c1 = _search(a4, g4, q, tau, 4)
        h8, l8, b8, op8, d0, d1 = _search(a8, g8, q, tau, 8)
        # strict: the window is clear (asserted by make_data) -- or, at 100 rows, every row is a candidate of both widths and fits
        clear = (n >= 4096 and name != "empty" and tau >= 0.62) or n == 100
        print(f"{n}x{d} {metric} {name} tau={tau}: inside eps {inside[name]}, bits {b4}/{b8}, operand {op4}/{op8}, clear {clear}, "
              f"nibble scans {c0['nibble_scans']} -> {c1['nibble_scans']}, reruns {c0['nibble_reruns']} -> {c1['nibble_reruns']}, "
              f"lambda_q {l4!r}, hits {None if h4 is None else len(h4)}")
        assert h4 == h8 and l4 == l8                       # bit for bit
        assert b8 == 8 and d1["nibble_scans"] == d0["nibble_scans"] and d1["nibble_reruns"] == d0["nibble_reruns"]
        try:
            want, lq = ref.search(q, tau)
        except oracle_lib.ZeroLambda:
            want, lq = None, 0.0
        if want is None:
            assert name == "empty" and h4 is None and l4 == 0.0
            assert c1["zero_lambda"] == c0["zero_lambda"] + 1 and d1["zero_lambda"] == d0["zero_lambda"] + 1
        else:
            assert name != "empty"
            assert_hits_match(h4, want, ref.scores(q, tau, lq), rtol=RTOL)
            assert_hits_match(h8, want, ref.scores(q, tau, lq), rtol=RTOL)
            assert abs(l4 - lq) <= RTOL * abs(lq)
        assert c1["searches_with_rerun"] == c0["searches_with_rerun"]
        if tau < 0.4:
            assert b4 == 8 and c1["nibble_scans"] == c0["nibble_scans"]        # the coarse chain stays on the 8-bit tiles
        elif clear:
            assert b4 == 4 and op4 == "int8-high" and c1["nibble_scans"] == c0["nibble_scans"] + 1
            assert c1["nibble_reruns"] == c0["nibble_reruns"]
        else:
            # outcome-driven: the search MUST try the tiles and ends clean or redone on 8 bits; only behind a rerun seen on this
            # workspace may it skip them
            tried = c1["nibble_scans"] - c0["nibble_scans"]
            rerun = c1["nibble_reruns"] - c0["nibble_reruns"]
            allowed = ((1, 0, 4), (1, 1, 8)) + (((0, 0, 8),) if armed else ())
            assert (tried, rerun, b4) in allowed, (tried, rerun, b4, armed)
            armed = armed or rerun > 0
    del a4, g4, a8, g8


def test_alternating_widths_on_one_workspace_answer_like_a_fresh_index(oracle_lib):
    """4-bit and 8-bit searches alternately on ONE workspace: each answer is the one a freshly built index gives that query as
    its first search -- nothing of one width's scan (digits, scales, coefficient, candidate state) leaks into the other's."""
    import pyarrowspace_amd as asp
    X, gp, qs, _ = make_data(4133, 544, "l2")
    # (the fresh direction's searches last: at either width its scorer candidates may overflow, after which the workspace's next
    # searches take the coarse chain, or skip the tiles)
    seq = [("dense", 4), ("perturbed", 8), ("draw", 4), ("dense", 8), ("perturbed", 4), ("draw", 8), ("dense", 4), ("empty", 8), ("empty", 4)]
    fresh = {}
    for name, bits in set(seq):
        a2, g2 = asp.ArrowSpaceBuilder.build(gp, X)
        fresh[(name, bits)] = _search(a2, g2, qs[name], 0.62, bits)[:3]
        del a2, g2
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    c0 = aspace.search_counters()
    for name, bits in seq:
        got = _search(aspace, gl, qs[name], 0.62, bits)
        assert got[:2] == fresh[(name, bits)][:2], (name, bits)
        if name != "empty":
            assert got[2] == bits
            assert fresh[(name, 4)][:2] == fresh[(name, 8)][:2]
            c1 = aspace.search_counters()
            assert c1["nibble_reruns"] == c0["nibble_reruns"] and c1["searches_with_rerun"] == c0["searches_with_rerun"]


def test_isotropic_rows_rerun_on_8_bits_and_skip_the_tiles_afterwards(oracle_lib):
    """Isotropic rows (no clusters: every cosine within a few hundredths of zero, far inside the nibble window) under forced 4 --
    an index large enough for the automatic rule has 400 000 rows, too many for a test of seconds.  The first search finds its
    candidates do not fit, is redone on the 8-bit tiles and answers correctly; nibble_reruns rises by one; the next search does
    not try the tiles."""
    import pyarrowspace_amd as asp
    n, d = 16384, 512
    rng = np.random.default_rng(11)
    X = _unit(rng.standard_normal((n, d)))
    gp = {"eps": calibrate_eps(X, 10, "l2"), "k": 10, "topk": TOPK, "p": 2.0, "sigma": None, "metric": "l2"}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    ref = oracle_lib.OracleIndex(X, gp)
    q1 = _unit(X[5] + 0.02 * rng.standard_normal(d) / np.sqrt(d))
    q2 = _unit(X[77] + 0.02 * rng.standard_normal(d) / np.sqrt(d))
    h1, l1, b1, _, c0, c1 = _search(aspace, gl, q1, 0.62, 4)
    print("first:", b1, c0, c1)
    want, lq = ref.search(q1, 0.62)
    assert_hits_match(h1, want, ref.scores(q1, 0.62, lq), rtol=RTOL)
    assert c1["nibble_scans"] == c0["nibble_scans"] + 1 and c1["nibble_reruns"] == c0["nibble_reruns"] + 1 and b1 == 8
    _set_bits(4)
    c2 = aspace.search_counters()
    h2 = aspace.search(q2, gl, 0.62)
    b2, c3 = aspace.last_scan_bits, aspace.search_counters()
    print("second:", b2, c2, c3)
    want2, lq2 = ref.search(q2, 0.62)
    assert_hits_match(h2, want2, ref.scores(q2, 0.62, lq2), rtol=RTOL)
    assert b2 == 8 and c3["nibble_scans"] == c2["nibble_scans"] and c3["nibble_reruns"] == c2["nibble_reruns"]
