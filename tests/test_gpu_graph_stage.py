"""GPU: the graph stage (csr_from_knn, energy_kernel, median_lambda_n, graph_shard_csr / _energy / _lambdas,
graph_from_knn_global) on hand-built neighbour lists and hand-made energy vectors, against oracle/oracle_np.py.

The lists are subsets of pairs of real items (key / dist / gy from oracle_np.pair_quantities, order (key, id) as S3
leaves them), so that rows far longer than k, rows that exist only through reverse entries, mutual next to one-sided
pairs, the scan's block edges, an empty graph, duplicates, a zero item and wide lists are reached without a k-NN pass
having to produce them.  The whole-graph routes do not validate their lists: every id fed here is in range.

The generators need no GPU (tests/test_graph_stage_inputs.py checks on the CPU that every case is well conditioned:
the 1e-9 below is test_gpu_parity.py's RTOL, and an ulp on every weight moves no output by more than 1e-11)."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import clustered
from oracle import oracle_np

pytestmark = pytest.mark.gpu

RTOL = 1e-9          # test_gpu_parity.py's
D = 16
PARAM_SETS = [("l2", "gaussian", 2.0), ("cosine", "rational", 2.0), ("l2", "gaussian", 1.5)]
HUB_CUTS = [0, 1, 2050, 2051, 4100]
HUB_SLICE = (700, 1900)


# ------------------------------------------------------------------------------------------------ list generators
def lists_from_neighbours(X, metric, nbrs):
    """nbrs[i]: the ids row i lists (in range, no self, no repeat).  -> (n64, lists) with lists[i] = (idx, key, dist, gy)
    in fp64 from oracle_np.pair_quantities, ordered by (key asc, id asc)."""
    m = oracle_np.METRIC_L2 if metric == "l2" else oracle_np.METRIC_COSINE
    n64 = np.einsum("ij,ij->i", X, X)
    lists = []
    for i, js in enumerate(nbrs):
        js = np.asarray(js, dtype=np.int64)
        assert len(set(js.tolist())) == len(js) and i not in js and (len(js) == 0 or (js.min() >= 0 and js.max() < X.shape[0]))
        key, dist, gy = oracle_np.pair_quantities(X[i], X[js], n64[i], n64[js], m)
        o = np.lexsort((js, key))
        lists.append((js[o], key[o], dist[o], gy[o]))
    return n64, lists


def graph_params(metric, kernel, p, k, lists):
    """eps above the largest key used, sigma = the median of the list distances (1.0 for lists without an entry)."""
    keys = np.concatenate([l[1] for l in lists]) if lists else np.zeros(0)
    dists = np.concatenate([l[2] for l in lists]) if lists else np.zeros(0)
    kmax = float(keys.max()) if len(keys) else 1.0
    eps = 1.01 * (np.sqrt(kmax) if metric == "l2" else kmax) + 1e-3
    sigma = float(np.median(dists)) if len(dists) else 1.0
    return {"eps": float(eps), "k": int(k), "topk": 5, "p": float(p), "sigma": sigma, "metric": metric, "kernel": kernel}


def pack_lists(lists, k, pad="plain"):
    """idx int32 [n][k], dist / gy fp64 [n][k], cnt int32 [n].  pad "plain": -1 / 0.0 beyond cnt; "poison": the row's
    own id (in range) and NaN."""
    n = len(lists)
    if pad == "plain":
        idx = np.full((n, k), -1, dtype=np.int32)
        dist, gy = np.zeros((n, k)), np.zeros((n, k))
    else:
        idx = np.repeat(np.arange(n, dtype=np.int32)[:, None], k, axis=1)
        dist, gy = np.full((n, k), np.nan), np.full((n, k), np.nan)
    cnt = np.zeros(n, dtype=np.int32)
    for i, (js, _, dd, gg) in enumerate(lists):
        c = len(js)
        assert c <= k
        idx[i, :c], dist[i, :c], gy[i, :c], cnt[i] = js, dd, gg, c
    return idx, dist, gy, cnt


def hub_neighbours(n=4100, k=8, seed=11):
    """Hubs 0, 2050 and n - 1 sit in the list of every row with i % 3 != 0; rows with i % 7 == 0 list nothing (row 0 is a
    hub that exists through reverse entries alone); pairs (2t, 2t + 1) with t % 4 == 0 list each other; the other entries
    are random one-sided ones, never an id divisible by 5 -- so the rows i % 35 == 0 (but 0) have no entry at all."""
    rng = np.random.default_rng(seed)
    hubs = (0, 2050, n - 1)
    cnt = rng.integers(0, k + 1, n)
    cnt[np.arange(n) % 7 == 0] = 0
    pool = np.array([j for j in range(n) if j % 5 != 0])
    nbrs = []
    for i in range(n):
        if i % 7 == 0:
            nbrs.append([])
            continue
        forced = [h for h in hubs if h != i] if i % 3 != 0 else []
        mate = i ^ 1
        if (i // 2) % 4 == 0 and mate < n and mate % 7 != 0 and mate not in forced:
            forced.append(mate)
        js = list(forced)
        want = max(int(cnt[i]), len(js))
        while len(js) < want:
            j = int(pool[rng.integers(0, len(pool))])
            if j != i and j not in js:
                js.append(j)
        nbrs.append(js)
    return nbrs


def ring_neighbours(n, k):
    """i -> i + 1 (k = 1), i -> i + 1, i + 2 (k = 3: one slot of padding) mod n; n = 1 lists nothing."""
    out = []
    for i in range(n):
        js = []
        for s in ((1,) if k == 1 else (1, 2)):
            j = (i + s) % n
            if j != i and j not in js:
                js.append(j)
        out.append(js)
    return out


def random_neighbours(n, k, seed, zero_rows=()):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = 0 if i in zero_rows else int(rng.integers(0, k + 1))
        js = rng.choice(n - 1, size=min(c, n - 1), replace=False)
        out.append((js + (js >= i)).tolist())
    return out


def duplicate_items(seed=5):
    """64 items: (0, 1), (2, 3), (4, 5) are exact duplicates.  0 and 1 list only each other and nobody lists them; 2 and 3
    list each other and 2 also lists 8 and 9; 4 and 5 list each other and 10, 11 list 5 (reverse entries only).  Rows 8..63
    form a ring."""
    X = clustered(64, D, nclust=3, seed=seed)
    X[1], X[3], X[5] = X[0], X[2], X[4]
    nbrs = [[] for _ in range(64)]
    nbrs[0], nbrs[1] = [1], [0]
    nbrs[2], nbrs[3] = [3, 8, 9], [2]
    nbrs[4], nbrs[5] = [5], [4]
    for i in range(8, 64):
        nbrs[i] = [8 + (i - 8 + 1) % 56, 8 + (i - 8 + 2) % 56]
    nbrs[10].append(5)
    nbrs[11].append(5)
    return X, nbrs, 4


def norm_items(seed=6):
    """300 items with row norms drawn from [0.5, 2]; item 17 is the zero vector, lists four items and is listed by others."""
    rng = np.random.default_rng(seed)
    X = clustered(300, D, nclust=6, seed=seed) * rng.uniform(0.5, 2.0, 300)[:, None]
    X[17] = 0.0
    nbrs = random_neighbours(300, 6, seed + 1)
    nbrs[17] = [3, 40, 41, 250]
    for i in (5, 99, 200):
        if 17 not in nbrs[i]:
            nbrs[i] = nbrs[i][:5] + [17]
    return X, nbrs, 6


@functools.lru_cache(maxsize=None)
def graph_case(name, metric="l2", kernel="gaussian", p=2.0):
    """-> (X, gp, n64, lists) of a named case; cached: the tests share the inputs and never write to them."""
    if name == "hubs":
        X, k = clustered(4100, D, nclust=6, seed=21), 8
        nbrs = hub_neighbours(4100, k)
    elif name.startswith("ring"):           # "ring<n>k<k>"
        n, k = (int(v) for v in name[4:].split("k"))
        X, nbrs = clustered(n, D, nclust=6, seed=100 + n), ring_neighbours(n, k)
    elif name == "empty":
        X, k = clustered(1025, D, nclust=6, seed=22), 4
        nbrs = [[] for _ in range(1025)]
    elif name == "duplicates":
        X, nbrs, k = duplicate_items()
    elif name == "norms":
        X, nbrs, k = norm_items()
    elif name == "wide":
        X, k = clustered(600, D, nclust=6, seed=23), 64
        nbrs = random_neighbours(600, k, 24)
    else:
        raise KeyError(name)
    n64, lists = lists_from_neighbours(X, metric, nbrs)
    return X, graph_params(metric, kernel, p, k, lists), n64, lists


RING_SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]
CASES = ([("hubs",) + ps for ps in PARAM_SETS]
         + [("ring%dk%d" % (n, k), m, kn, 2.0) for n in RING_SIZES for k in (1, 3) for m, kn in (("l2", "gaussian"), ("cosine", "rational"))]
         + [("empty", "l2", "gaussian", 2.0)]
         + [(c, m, kn, 2.0) for c in ("duplicates", "norms", "wide") for m, kn in (("l2", "gaussian"), ("cosine", "rational"))])


@functools.lru_cache(maxsize=None)
def oracle_graph(case):
    X, gp, n64, lists = graph_case(*case)
    return oracle_np.graph_from_lists(X, oracle_np.resolve_params(gp), n64, lists)


def incoming_edges(lists, lo, hi):
    """Every directed edge of the whole graph whose target row lives in [lo, hi): (local row, source, dist, gy) arrays, in
    the lists' (row, slot) order."""
    rows, src, dd, gg = [], [], [], []
    for i, (js, _, dist, gy) in enumerate(lists):
        here = (js >= lo) & (js < hi)
        rows.append(js[here] - lo)
        src.append(np.full(int(here.sum()), i, dtype=np.int64))
        dd.append(dist[here])
        gg.append(gy[here])
    return tuple(np.concatenate(v) if v else np.zeros(0) for v in (rows, src, dd, gg))


# ------------------------------------------------------------------------------------------------ energy vectors (S8)
def _embed(rng, n, values, filler=(0.0, float("nan"), -1.0)):
    """`values` at random places of a length-n vector, the rest zeros / NaN / negatives: none of them is positive."""
    assert len(values) <= n
    E = np.asarray(filler)[rng.integers(0, len(filler), n)]
    E[rng.permutation(n)[: len(values)]] = values
    return E


def median_vectors(n_global, seed=0):
    """(name, E_global) pairs of length n_global for the selection.  Every size has the few-positives vectors; a size
    beyond 262144 (= 1024 blocks x 256 threads of the histogram kernel) has one vector alone, whose every positive sits
    beyond that index; a size of 1000 to 262144 also carries the last-bytes, ties and clamp vectors, which need about 400
    slots -- MEDIAN_SIZES holds 1000 for them, and tests/test_graph_stage_inputs.py asserts that their names occur."""
    rng = np.random.default_rng(seed + n_global)
    n, out = n_global, []
    if n > 262144:
        E = np.zeros(n)
        E[:262144:3] = np.nan
        E[262144:] = rng.uniform(1e-6, 0.9, n - 262144)
        return [("positives_beyond_one_grid", E)]
    if n <= 8:
        out += [("zeros", np.zeros(n)), ("negatives", -rng.uniform(0.1, 1.0, n)), ("nan", np.full(n, np.nan)),
                ("mixed_nonpositive", np.array([0.0, -0.0, np.nan, -3.0] * n)[:n])]
        for c in range(1, min(n, 5) + 1):
            out.append(("%d_positive" % c, _embed(rng, n, rng.uniform(0.01, 0.9, c))))
    else:
        for c in (1, 2, 3, 4, 5):
            out.append(("%d_positive" % c, _embed(rng, n, rng.uniform(0.01, 0.9, c))))
        out.append(("random", _embed(rng, n, rng.uniform(1e-6, 0.9, n // 2))))
        out.append(("all_positive", rng.uniform(1e-6, 0.9, n)))
    if n >= 1000:
        chain = [0.3]
        for _ in range(299):
            chain.append(np.nextafter(chain[-1], 1.0))
        chain = np.array(chain)
        assert (chain.view(np.uint64) >> 8).min() != (chain.view(np.uint64) >> 8).max()      # crosses a byte boundary
        out.append(("last_bytes_300", _embed(rng, n, rng.permutation(chain))))
        out.append(("last_bytes_299", _embed(rng, n, rng.permutation(chain[:299]))))
        m = 150
        lo_v, hi_v, a, b = rng.uniform(0.01, 0.1, m), rng.uniform(0.5, 0.9, m), 0.25, 0.26
        out.append(("tie_across_rank", _embed(rng, n, np.concatenate([lo_v, np.full(101, a), hi_v]))))
        out.append(("tie_m_m", _embed(rng, n, np.concatenate([np.full(m, a), np.full(m, b)]))))
        out.append(("tie_m_m1", _embed(rng, n, np.concatenate([np.full(m, a), np.full(m + 1, b)]))))
        out.append(("tie_m1_m", _embed(rng, n, np.concatenate([np.full(m + 1, a), np.full(m, b)]))))
        den = np.array([5e-324, 1e-310, 2.5e-308])
        out.append(("wide_range", _embed(rng, n, np.concatenate([10.0 ** rng.uniform(-300, 300, 400), den]))))
        out.append(("clamp_low", _embed(rng, n, np.concatenate([10.0 ** rng.uniform(-300, -13, 300), den, [0.5, 2.0]]))))
        out.append(("clamp_high", _embed(rng, n, np.concatenate([10.0 ** rng.uniform(0.5, 300, 300), den, [0.5, 1e-20]]))))
        out.append(("just_below_tau_min", _embed(rng, n, np.array([np.nextafter(1e-12, 0.0)] * 3 + [1e-300, 0.7]))))
    return out


MEDIAN_SIZES = [4, 255, 256, 257, 1000, 262144 + 257]       # 1000: the size that carries the last-bytes, ties and clamp vectors


def median_shard_inputs():
    """The 4-row shard the crafted energy vectors are selected for: a ring among 4 items (k = 2) and its reverse edges."""
    X = clustered(4, D, nclust=2, seed=31)
    n64, lists = lists_from_neighbours(X, "l2", [[(i + 1) % 4, (i + 2) % 4] for i in range(4)])
    return X, graph_params("l2", "gaussian", 2.0, 2, lists), n64, lists


# ------------------------------------------------------------------------------------------------ GPU side
# tests/test_graph_stage_inputs.py imports this module on machines without a GPU: nothing at module level may import
# torch or pyarrowspace_amd or touch a device; the helpers and tests below import them where they run.
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _engine(gp, X):
    from pyarrowspace_amd.dist import HipEngine
    e = HipEngine(gp)
    e.create_space(_dev(X))
    return e


def _csr(e):
    """(indptr, indices, values) through as_graph_csr (diagonal included)."""
    L = e.L
    rows, nnz = int(L.as_nnodes(e.gr)), int(L.as_graph_nnz(e.gr))
    ip, ix, v = np.zeros(rows + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64), np.zeros(max(nnz, 1))
    e._check(L.as_graph_csr(e.gr, ip.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)))
    assert ip[rows] == nnz
    return ip, ix[:nnz], v[:nnz]


def _rows_vec(e, fn):
    """as_graph_deg_copy / as_graph_energy_copy: one double per row of the GRAPH (not of the space: the global route's
    graph has n_global rows on a space of fewer)."""
    import torch
    rows = int(e.L.as_nnodes(e.gr))
    out = torch.zeros((max(rows, 1),), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e._check(fn(e.gr, C.c_void_p(out.data_ptr())))
    return out[:rows].cpu().numpy()


def _outputs(e):
    ip, ix, v = _csr(e)
    return dict(indptr=ip, indices=ix, values=v, deg=_rows_vec(e, e.L.as_graph_deg_copy), E=_rows_vec(e, e.L.as_graph_energy_copy),
                tau0=e.tau0(), lambdas=e.lambdas().copy())


def _reldiff(got, want):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    if got.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    r[(got == want)] = 0.0
    return float(np.max(r))


def _check_rows(out, ref, lo, hi, lam_lo=None, lam_hi=None, label=""):
    """GPU rows [lo, hi) of the graph (column ids global, diagonal at column lo + r) against the oracle's, the way
    test_gpu_parity.py's _check_index does; lambdas of rows [lam_lo, lam_hi)."""
    n = hi - lo
    ip, ix, v = out["indptr"], out["indices"], out["values"]
    rows = np.repeat(np.arange(n), np.diff(ip)) + lo
    off = ix != rows
    rip = ref["indptr"]
    assert np.array_equal(np.bincount(rows[off] - lo, minlength=n), np.diff(rip[lo : hi + 1]))        # indptr, exact
    assert np.array_equal(np.bincount(rows[~off] - lo, minlength=n), np.ones(n, dtype=np.int64))      # one diagonal entry per row
    assert np.array_equal(ix[off], ref["indices"][rip[lo] : rip[hi]])
    figures = dict(lap=_reldiff(v[off], ref["lap"][rip[lo] : rip[hi]]), deg=_reldiff(out["deg"], ref["deg"][lo:hi]),
                   E=_reldiff(out["E"], ref["E"][lo:hi]), tau0=_reldiff(out["tau0"], ref["tau0"]))
    lam_lo, lam_hi = (lo, hi) if lam_lo is None else (lam_lo, lam_hi)
    figures["lambda"] = _reldiff(out["lambdas"], ref["lambdas"][lam_lo:lam_hi])
    print("graph-stage %s rows [%d, %d): " % (label, lo, hi) + " ".join("%s=%.3g" % kv for kv in figures.items()))
    np.testing.assert_allclose(v[off], ref["lap"][rip[lo] : rip[hi]], rtol=RTOL, atol=1e-300)
    np.testing.assert_array_equal(v[~off], (ref["deg"][lo:hi] > 0).astype(np.float64))
    np.testing.assert_allclose(out["deg"], ref["deg"][lo:hi], rtol=RTOL, atol=1e-300)
    np.testing.assert_allclose(out["E"], ref["E"][lo:hi], rtol=RTOL, atol=1e-300)
    assert abs(out["tau0"] - ref["tau0"]) <= RTOL * abs(ref["tau0"])
    np.testing.assert_allclose(out["lambdas"], ref["lambdas"][lam_lo:lam_hi], rtol=RTOL, atol=1e-300)


def _run_whole(case, pad="plain"):
    X, gp, _, lists = graph_case(*case)
    e = _engine(gp, X)
    e.graph_from_knn(*[_dev(a) for a in pack_lists(lists, gp["k"], pad)])
    return e


def _check_whole(case):
    ref = oracle_graph(case)
    e = _run_whole(case)
    out = _outputs(e)
    e.close()
    n = len(ref["deg"])
    assert out["tau0"] == oracle_np.median_tau(out["E"])        # a selection does no arithmetic: the GPU's own median, bit for bit
    _check_rows(out, ref, 0, n, label="/".join(str(c) for c in case))
    return out, ref


# ------------------------------------------------------------------------------------------------ A. the cases
@pytest.mark.parametrize("metric,kernel,p", PARAM_SETS)
def test_hubs_three_routes_match_oracle_and_each_other(metric, kernel, p):
    """Rows of thousands of reverse entries, rows without an own list, mutual next to one-sided pairs, four scan blocks:
    as_graph_from_knn, as_graph_from_knn_global (a space of rows [700, 1900)) and the sharded stage (two shards are a hub
    row alone) against the oracle at 1e-9, and against one another bit for bit."""
    import torch
    case = ("hubs", metric, kernel, p)
    X, gp, _, lists = graph_case(*case)
    n, k = X.shape[0], gp["k"]
    ref = oracle_graph(case)
    packed = [_dev(a) for a in pack_lists(lists, k)]
    # route 1: one space holding everything
    whole = _engine(gp, X)
    whole.graph_from_knn(*packed)
    out_w = _outputs(whole)
    n64_dev = whole.norms().contiguous()
    assert out_w["tau0"] == oracle_np.median_tau(out_w["E"])
    _check_rows(out_w, ref, 0, n, label="hubs/whole")
    # route 2: the global graph on a space that holds rows [700, 1900) only (the lambda slice)
    lo, hi = HUB_SLICE
    part = _engine(gp, X[lo:hi])
    part.graph_from_knn_global(n, lo, *packed, n64_dev)
    out_g = _outputs(part)
    assert out_g["tau0"] == oracle_np.median_tau(out_g["E"])
    _check_rows(out_g, ref, 0, n, lo, hi, label="hubs/global")
    for key in ("indptr", "indices", "values", "deg", "E"):
        np.testing.assert_array_equal(out_g[key], out_w[key])
    assert out_g["tau0"] == out_w["tau0"]
    np.testing.assert_array_equal(out_g["lambdas"], out_w["lambdas"][lo:hi])
    part.close()
    # route 3: row shards; every shard receives the directed edges whose target row it owns
    prm = oracle_np.resolve_params(gp)
    shards = []
    for lo, hi in zip(HUB_CUTS[:-1], HUB_CUTS[1:]):
        e = _engine(gp, X[lo:hi])
        r, s, dd, gg = incoming_edges(lists, lo, hi)
        deg = e.graph_shard_csr(n, lo, *[t[lo:hi].contiguous() for t in packed], _dev(r.astype(np.int32)), _dev(s.astype(np.int32)),
                                _dev(dd), _dev(gg))
        sh = oracle_np.shard_csr(prm, lo, hi - lo, lists[lo:hi], zip(r, s, dd, gg))
        shards.append((e, deg, sh))
    deg_g = torch.cat([dg for _, dg, _ in shards]).contiguous()
    np.testing.assert_array_equal(deg_g.cpu().numpy(), out_w["deg"])
    E_g = torch.cat([e.graph_shard_energy(deg_g, n64_dev) for e, _, _ in shards]).contiguous()
    np.testing.assert_array_equal(E_g.cpu().numpy(), out_w["E"])
    deg_ref = np.concatenate([sh["deg"] for _, _, sh in shards])
    np.testing.assert_array_equal(deg_ref, ref["deg"])
    for (e, _, sh), lo, hi in zip(shards, HUB_CUTS[:-1], HUB_CUTS[1:]):
        e.graph_shard_lambdas(E_g)
        out = _outputs(e)
        assert out["tau0"] == out_w["tau0"]
        assert int(e.L.as_graph_row_offset(e.gr)) == lo and int(e.L.as_graph_ncols(e.gr)) == n
        _check_rows(out, ref, lo, hi, label="hubs/shard")
        # the oracle's own shard functions, fed the oracle's global degrees
        oracle_np.shard_energy(sh, deg_ref, ref["n"])
        rows = np.repeat(np.arange(hi - lo), np.diff(out["indptr"])) + lo
        off = out["indices"] != rows
        assert np.array_equal(out["indices"][off], sh["indices"])
        np.testing.assert_allclose(out["values"][off], sh["lap"], rtol=RTOL, atol=1e-300)
        np.testing.assert_allclose(out["deg"], sh["deg"], rtol=RTOL, atol=1e-300)
        np.testing.assert_allclose(out["E"], sh["E"], rtol=RTOL, atol=1e-300)
        # bit for bit the whole graph's rows
        ipw = out_w["indptr"]
        np.testing.assert_array_equal(out["indptr"], ipw[lo : hi + 1] - ipw[lo])
        np.testing.assert_array_equal(out["indices"], out_w["indices"][ipw[lo] : ipw[hi]])
        np.testing.assert_array_equal(out["values"], out_w["values"][ipw[lo] : ipw[hi]])
        np.testing.assert_array_equal(out["lambdas"], out_w["lambdas"][lo:hi])
        e.close()
    whole.close()


@pytest.mark.parametrize("n", RING_SIZES)
def test_ring_lists_at_scan_and_row_tile_edges(n):
    """Row counts around the 256-row launch tiles and the 1024-row scan blocks; k = 1 (no padding) and k = 3."""
    for k in (1, 3):
        for metric, kernel in (("l2", "gaussian"), ("cosine", "rational")):
            out, ref = _check_whole(("ring%dk%d" % (n, k), metric, kernel, 2.0))
            if n == 1:
                assert len(out["indices"]) == 1 and out["values"][0] == 0.0 and out["tau0"] == oracle_np.TAU_MIN and out["lambdas"][0] == 0.0


def test_graph_without_any_edge():
    case = ("empty", "l2", "gaussian", 2.0)
    out, ref = _check_whole(case)
    n = 1025
    np.testing.assert_array_equal(out["indptr"], np.arange(n + 1))
    np.testing.assert_array_equal(out["indices"], np.arange(n))
    np.testing.assert_array_equal(out["values"], np.zeros(n))
    np.testing.assert_array_equal(out["deg"], np.zeros(n))
    assert out["tau0"] == 1e-12
    np.testing.assert_array_equal(out["lambdas"], np.zeros(n))


def test_entries_beyond_cnt_are_never_read():
    """The hub lists padded with -1 / 0.0, then with the row's own id and NaN: every output bit-identical."""
    # one metric / kernel is enough: the kernels that read idx and cnt (sym_count / sym_fill) do not depend on either
    case = ("hubs", "l2", "gaussian", 2.0)
    outs = []
    for pad in ("plain", "poison"):
        e = _run_whole(case, pad)
        outs.append(_outputs(e))
        e.close()
    for key in ("indptr", "indices", "values", "deg", "E", "lambdas"):
        np.testing.assert_array_equal(outs[0][key], outs[1][key])
    assert outs[0]["tau0"] == outs[1]["tau0"]
    assert np.isfinite(outs[1]["lambdas"]).all()


@pytest.mark.parametrize("metric,kernel", [("l2", "gaussian"), ("cosine", "rational")])
def test_identical_neighbours(metric, kernel):
    out, ref = _check_whole(("duplicates", metric, kernel, 2.0))
    # 0 and 1 are duplicates that list only each other: equal degrees, S = 0, out of the median
    assert out["deg"][0] == out["deg"][1] and out["E"][0] == 0.0 and out["E"][1] == 0.0
    assert out["lambdas"][0] == 0.0 and out["lambdas"][1] == 0.0
    # 2 / 3 and 4 / 5 are duplicates of unequal degree: a positive energy
    assert out["deg"][2] != out["deg"][3] and out["E"][2] > 0.0 and out["E"][3] > 0.0
    assert out["deg"][4] != out["deg"][5] and out["E"][4] > 0.0 and out["E"][5] > 0.0


@pytest.mark.parametrize("metric,kernel", [("l2", "gaussian"), ("cosine", "rational")])
def test_unequal_norms_and_a_zero_item(metric, kernel):
    out, ref = _check_whole(("norms", metric, kernel, 2.0))
    assert out["deg"][17] > 0.0 and out["E"][17] == 0.0        # the zero item has neighbours and no energy of its own (ny = 0)


@pytest.mark.parametrize("metric,kernel", [("l2", "gaussian"), ("cosine", "rational")])
def test_wide_lists(metric, kernel):
    _check_whole(("wide", metric, kernel, 2.0))


# ------------------------------------------------------------------------------------------------ B. the median
@pytest.mark.parametrize("n_global", MEDIAN_SIZES)
def test_median_of_hand_made_energies(n_global):
    """as_graph_shard_lambdas selects tau0 over an arbitrary energy vector: bit-equal to the sorted lower median, clamped;
    the shard's 4 lambdas follow from its own E / G and that tau0."""
    X, gp, n64, lists = median_shard_inputs()
    prm = oracle_np.resolve_params(gp)
    r, s, dd, gg = incoming_edges(lists, 0, 4)
    sh = oracle_np.shard_csr(prm, 0, 4, lists, zip(r, s, dd, gg))
    deg_global, n64_global = np.ones(n_global), np.ones(n_global)
    deg_global[:4], n64_global[:4] = sh["deg"], n64
    E_own, G_own = oracle_np.shard_energy(sh, deg_global, n64_global)
    assert (E_own > 0).all() and (G_own > 0).all()
    e = _engine(gp, X)
    deg = e.graph_shard_csr(n_global, 0, *[_dev(a) for a in pack_lists(lists, 2)], _dev(r.astype(np.int32)), _dev(s.astype(np.int32)),
                            _dev(dd), _dev(gg))
    np.testing.assert_allclose(deg.cpu().numpy(), sh["deg"], rtol=RTOL)
    E_gpu = e.graph_shard_energy(_dev(deg_global), _dev(n64_global)).cpu().numpy()       # before _lambdas: it allocates E and G
    np.testing.assert_allclose(E_gpu, E_own, rtol=RTOL)
    vectors = median_vectors(n_global)
    assert vectors
    for name, E_global in vectors:
        assert E_global.shape == (n_global,)
        want = oracle_np.median_tau(E_global)
        e.graph_shard_lambdas(_dev(E_global))
        got = e.tau0()
        assert got == want, (name, n_global, got, want)
        np.testing.assert_allclose(e.lambdas(), oracle_np.synth_lambda(E_own, G_own, want), rtol=RTOL, atol=1e-300, err_msg=name)
    e.close()
