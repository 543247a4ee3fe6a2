"""GPU: non-finite items through every filtered form (sections 5.9-5.17) -- score_items, search_subset, their
batched, per-query-list and tau-sweep forms, range, fused, grouped and diversified search over indexes whose items carry +inf,
-inf, NaN, all-NaN and all-zero rows, a run of consecutive inf rows that covers whole waves (and, at 3000 rows, more than the
1024 entries one block sorts) and rows of huge finite values whose dot product overflows for one query only.  What the fixtures
contain is asserted without a GPU by tests/test_filtered_nonfinite_inputs.py.

Expected values: the NaN mask is the fp64 oracle's, exactly; finite scores agree with the oracle under the tolerance of
tests/test_gpu_subset.py (RTOL, atol_for); everything else is bit-equality with the numpy route over the form's own scores:
number before NaN, score descending (-0.0 and +0.0 tying), index ascending.  NaN scores are compared as NaN, not by payload."""
import numpy as np
import pytest

import diverse_ref
import fused_ref
import grouped_ref
from conftest import calibrate_eps, clustered

RTOL = 1e-9   # tests/test_gpu_parity.py's
TAUS = (1.0, 0.62, 0.0, 1.5)
NVEC = 66     # one past the batched score kernel's query tile, and one more
ZCOL = 5      # the column in which the queries are exactly 0
HUGE = 1.7e308   # the overflow rows: HUGE in two columns, elsewhere 0; the one query with 0.6 * 1.01 in both overflows the dot
HCOLS = ((6, 7), (8, 10), (12, 13))   # ... the columns of overflow row h; every other query is exactly 0 in all six

# (n, d, k, topk, metric, kernel, rounded through float32, first and last row of the inf run, overflow rows)
SHAPES = {"3000x51": (3000, 51, 8, 1024, "l2", "gaussian", False, (1500, 2600), True),
          "3000x96cos": (3000, 96, 25, 1024, "cosine", "rational", False, (1500, 2600), True),
          "700x768f32": (700, 768, 12, 64, "l2", "gaussian", True, (300, 370), False)}
_data, _built = {}, {}


def atol_for(d):
    """tests/test_gpu_subset.py's: the fp64 dot error of unit-norm rows."""
    return 16 * d * 2.0 ** -53


def poisoned(name):
    """The fixture of a shape, made on the host: dict with X (poisoned), clean (before poisoning), gp, the poisoned rows by kind,
    `nan_rows` (rows whose score is NaN for every query: an inf anywhere), `lam_rows` (rows that score their lambda term: NaN or
    zero norm), `huge` (row h: NaN for query h alone) and `qrows`, the clean rows the queries are made of."""
    if name in _data:
        return _data[name]
    n, d, k, topk, metric, kernel, f32, (r0, r1), with_huge = SHAPES[name]
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64)) if f32 else X * (1 + 1e-9)   # fp32 rows / fp64 rows kept
    rows = {"pinf": [0, 63, 64, 255, 256, n - 1], "ninf": [128], "run": list(range(r0, r1)), "nan": [1, 65, 257],
            "allnan": [200], "zero": [201], "inf_at_zcol": [129], "huge": [130, 131, 132] if with_huge else []}
    bad = sorted(r for v in rows.values() for r in v)
    assert len(set(bad)) == len(bad)
    rng = np.random.default_rng(n + 7 * d)
    good = [int(r) for r in rng.permutation(n) if r not in set(bad)]
    qrows, spare = good[:2 * NVEC], good[2 * NVEC:]
    X[qrows, ZCOL] = 0.0   # the queries are these rows x 1.01: exactly 0 in ZCOL, so an inf there meets a 0
    if with_huge:
        X[np.ix_(qrows, [c for pair in HCOLS for c in pair])] = 0.0
        for h, pair in enumerate(HCOLS):
            X[qrows[h], list(pair)] = 0.6
            mates = spare[6 * h:6 * h + 6]   # six near copies: the row keeps neighbours inside eps, its query a lambda_q
            X[mates] = X[qrows[h]] + 0.01 * rng.standard_normal((6, d))
    clean = X.copy()
    gp = {"eps": calibrate_eps(clean, k, metric), "k": k, "topk": topk, "p": 2.0, "sigma": None, "metric": metric, "kernel": kernel}
    for t, r in enumerate(rows["pinf"]):
        X[r, (3 + 7 * t) % d] = np.inf
    X[rows["ninf"][0], 9] = -np.inf
    for r in rows["run"]:
        X[r, r % d] = np.inf
    for t, r in enumerate(rows["nan"]):
        X[r, (11 + 5 * t) % d] = np.nan
    X[rows["allnan"][0]] = np.nan
    X[rows["zero"][0]] = 0.0
    X[rows["inf_at_zcol"][0], ZCOL] = np.inf
    for h, r in enumerate(rows["huge"]):   # its dot with query h is 2 * HUGE * 0.606 = inf over a norm of inf: NaN; with any other, 0
        X[r] = 0.0
        X[r, list(HCOLS[h])] = HUGE
    nan_rows = sorted(rows["pinf"] + rows["ninf"] + rows["run"] + rows["inf_at_zcol"])
    lam_rows = sorted(rows["nan"] + rows["allnan"] + rows["zero"])
    _data[name] = {"X": np.ascontiguousarray(X), "clean": clean, "gp": gp, "rows": rows, "nan_rows": nan_rows, "lam_rows": lam_rows,
                   "huge": rows["huge"], "qrows": qrows, "bad": bad}
    return _data[name]


def queries(name, served):
    """NVEC queries, clean rows x 1.01, whose lambda_q is not 0 under `served`; the first three are those of the overflow rows."""
    fx = poisoned(name)
    vecs = []
    for r in fx["qrows"]:
        q = np.ascontiguousarray(fx["clean"][r] * 1.01)
        assert q[ZCOL] == 0.0
        if len(vecs) < len(fx["huge"]) or served(q):
            vecs.append(q)
        if len(vecs) == NVEC:
            break
    assert len(vecs) == NVEC
    return np.stack(vecs)


def np_order(ids, s, k=None):
    """Positions of the first k entries by (number before NaN, score descending with -0.0 == +0.0, index ascending)."""
    ids, s = np.asarray(ids, dtype=np.int64), np.asarray(s, dtype=np.float64)
    nan = np.isnan(s)
    return np.lexsort((ids, -(np.where(nan, 0.0, s) + 0.0), nan))[:k]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_scores(got, want):
    """Equal NaN masks, equal bits elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got[ok]), bits(want[ok]))


def same_hits(got, ids, s, k):
    """A hit list against the numpy order over (ids, s)."""
    o = np_order(ids, s, k)
    assert [i for i, _ in got] == np.asarray(ids)[o].tolist()
    same_scores([v for _, v in got], np.asarray(s)[o])


def subsets(name):
    """The id sets of the selection cases: name -> sorted ids."""
    fx = poisoned(name)
    n, topk = fx["X"].shape[0], fx["gp"]["topk"]
    rng = np.random.default_rng(5)
    good = np.setdiff1d(np.arange(n), fx["bad"])
    run = np.asarray(fx["rows"]["run"])
    few = rng.choice(good, min(topk, 40) // 2, replace=False)   # fewer numbers than topk
    out = {"all": np.arange(n), "only poisoned": np.asarray(fx["bad"])[:1024] if len(fx["bad"]) <= 1024 else
           np.sort(np.concatenate([np.setdiff1d(fx["bad"], run), run[:900]])),
           "one-block mix": np.sort(np.concatenate([few, run[:min(len(run), 600)], fx["lam_rows"][:2], fx["rows"]["pinf"]]))}
    if len(run) > 1024:
        out["threshold inside the NaN run"] = np.sort(np.concatenate([few, run, fx["lam_rows"], fx["rows"]["pinf"]]))
        out["nothing but the NaN run"] = run
    return out


def index(name, topk=None):
    """One index per (shape, topk) for the whole module: (asp, fixture, gp, aspace, gl, NVEC queries, the oracle index)."""
    key = (name, topk)
    if key not in _built:
        import pyarrowspace_amd as asp
        from oracle import oracle_c
        fx = poisoned(name)
        gp = dict(fx["gp"], topk=fx["gp"]["topk"] if topk is None else topk)
        aspace, gl = asp.ArrowSpaceBuilder.build(gp, fx["X"])
        if (name, None) in _built:
            V, ref = _built[(name, None)][5], _built[(name, None)][6]
        else:
            ref = oracle_c.OracleIndex(fx["X"], gp)
            V = queries(name, lambda q: ref.query_lambda(q) != 0.0)
        _built[key] = (asp, fx, gp, aspace, gl, V, ref)
    return _built[key]


def oracle_scores(ref, q, tau):
    return ref.scores(q, tau, ref.query_lambda(q))


pytestmark = pytest.mark.gpu
NAMES = list(SHAPES)


def agrees_with_oracle(got, want, d):
    """The oracle's NaN mask exactly; its finite scores under tests/test_gpu_subset.py's tolerance."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.isfinite(got[ok]).all()
    np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL, atol=atol_for(d))


def query_lists(fx, B, rng):
    """B id lists in the caller's order, each with poisoned rows of every kind, of different lengths; one of a single id."""
    n = fx["X"].shape[0]
    lists = []
    for i in range(B):
        m = 1 if i == 1 else int(rng.integers(5, 400))
        ids = np.concatenate([rng.integers(0, n, m), rng.choice(fx["bad"], min(m, 7))]) if m > 1 else np.array([fx["nan_rows"][0]])
        rng.shuffle(ids)
        lists.append(ids.astype(np.int64))
    return lists


@pytest.mark.parametrize("name", NAMES)
def test_scores(name):
    """S11 per item: an inf anywhere in a row is a NaN score at every tau; a NaN or zero norm is cosine 0, the lambda term alone."""
    asp, fx, gp, aspace, gl, V, ref = index(name)
    n, d = fx["X"].shape
    every, lamr = np.arange(n), np.asarray(fx["lam_rows"])
    np.testing.assert_allclose(aspace.lambdas(), ref.lambdas, rtol=RTOL, atol=1e-300)
    assert (aspace.lambdas()[fx["bad"]] == 0.0).all()
    lqs = np.array([ref.query_lambda(q) for q in V])
    want = {tau: np.stack([ref.scores(q, tau, lq) for q, lq in zip(V, lqs)]) for tau in TAUS}
    masks = np.isnan(want[TAUS[0]])
    for h, r in enumerate(fx["huge"]):
        assert masks[h, r] and not masks[np.arange(NVEC) != h, r].any()   # the overflow row: NaN for its own query alone
    for j in (0, 1, 2, 7):
        sweep = aspace.score_items_taus(V[j], gl, TAUS, every)
        for u, tau in enumerate(TAUS):
            got = aspace.score_items(V[j], gl, tau, every)
            agrees_with_oracle(got, want[tau][j], d)
            assert np.array_equal(np.flatnonzero(np.isnan(got)), np.flatnonzero(masks[j]))
            np.testing.assert_allclose(got[lamr], (1.0 - tau) / (1.0 + np.abs(lqs[j])), rtol=RTOL)   # lambda_i = 0, cosine 0
            if tau == 1.0:
                assert not bits(got[lamr]).any()   # +0.0
            same_scores(sweep[u], got)
    rng = np.random.default_rng(11)
    lists = query_lists(fx, NVEC, rng)
    SL = aspace.score_lists_batch_taus(V, gl, TAUS, lists)
    SB = aspace.score_items_batch_taus(V, gl, TAUS, every)
    for u, tau in enumerate(TAUS):
        S = aspace.score_items_batch(V, gl, tau, every)
        agrees_with_oracle(S, want[tau], d)
        assert np.array_equal(np.isnan(S), masks)   # the single, batched and list forms agree on the mask
        if tau == 1.0:
            assert not bits(S[:, lamr]).any()
        same_scores(SB[:, u], S)
        L = aspace.score_lists_batch(V, gl, tau, lists)
        for i in range(NVEC):
            agrees_with_oracle(L[i], want[tau][i][lists[i]], d)
            same_scores(SL[i][u], L[i])


def selection_cases(name):
    asp, fx, gp, aspace, gl, V, ref = index(name)
    return [(case, ids, aspace.subset(ids)) for case, ids in subsets(name).items()]


@pytest.mark.parametrize("name", NAMES)
def test_selection(name):
    """Section 5.9 item 3: NaN ranks lowest, and among NaN entries the lower index comes first -- through the one-block sort, the
    radix select with its threshold inside a run of more than 1024 all-zero keys, the lists' one-block select, and the sweeps."""
    asp, fx, gp, aspace, gl, V, ref = index(name)
    topk = gp["topk"]
    numbers = set(fx["lam_rows"] + fx["huge"])
    for case, ids, sub in selection_cases(name):
        k = min(topk, len(ids))
        for j in (0, 5):
            sweep_s = aspace.score_items_taus(V[j], gl, TAUS, ids)
            sweep = aspace.search_subset_taus(V[j], gl, TAUS, sub)
            for u, tau in enumerate(TAUS):
                s = aspace.score_items(V[j], gl, tau, ids)
                got = aspace.search_subset(V[j], gl, tau, sub)
                assert len(got) == k
                same_hits(got, ids, s, k)
                same_hits(sweep[u], ids, sweep_s[u], k)
                if case == "only poisoned":   # every number is a lambda term; then the NaN entries in index order
                    nn = int((~np.isnan(s)).sum())
                    assert nn < k and all(i in numbers for i, _ in got[:nn]) and all(v != v for _, v in got[nn:])
                    assert [i for i, _ in got[nn:]] == sorted(i for i, _ in got[nn:])
                if case == "threshold inside the NaN run":
                    assert int((~np.isnan(s)).sum()) < k < len(ids) and len(ids) > 1024
        B = NVEC if case in ("all", "threshold inside the NaN run") else 3
        Q = V[:B]
        lists = [ids[::-1].copy() if i % 2 else ids for i in range(B)]   # (the lists' order is the caller's)
        for tau in (0.62, 1.0):
            S = aspace.score_items_batch(Q, gl, tau, ids)
            res = aspace.search_batch_subset(Q, gl, tau, sub)
            SL = aspace.score_lists_batch(Q, gl, tau, lists)
            resl = aspace.search_batch_lists(Q, gl, tau, lists)
            for i in range(B):
                same_hits(res[i], ids, S[i], k)
                same_hits(resl[i], lists[i], SL[i], k)
        Q = V[:3]
        S = aspace.score_items_batch_taus(Q, gl, TAUS, ids)
        res = aspace.search_batch_subset_taus(Q, gl, TAUS, sub)
        SL = aspace.score_lists_batch_taus(Q, gl, TAUS, lists[:3])
        resl = aspace.search_batch_lists_taus(Q, gl, TAUS, lists[:3])
        for i in range(3):
            for u in range(len(TAUS)):
                same_hits(res[i][u], ids, S[i, u], k)
                same_hits(resl[i][u], lists[i], SL[i][u], k)


@pytest.mark.parametrize("name", [nm for nm in NAMES if SHAPES[nm][0] == 3000])
def test_selection_of_one(name):
    """topk = 1: the radix select's threshold is the first key of the run, or the one number above it."""
    asp, fx, gp, aspace, gl, V, ref = index(name, 1)
    for case, ids in subsets(name).items():
        sub = aspace.subset(ids)
        for tau in (0.62, 1.0):
            s = aspace.score_items(V[0], gl, tau, ids)
            got = aspace.search_subset(V[0], gl, tau, sub)
            same_hits(got, ids, s, 1)
            if case == "nothing but the NaN run":
                assert got[0][0] == ids[0] and got[0][1] != got[0][1]
            same_hits(aspace.search_batch_subset(V[:2], gl, tau, sub)[1], ids, aspace.score_items_batch(V[:2], gl, tau, ids)[1], 1)
            same_hits(aspace.search_batch_lists(V[:2], gl, tau, [ids, ids])[1], ids, aspace.score_lists_batch(V[:2], gl, tau, [ids, ids])[1], 1)


def range_want(ids, s, thr):
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero(s >= thr)
    o = keep[np.lexsort((ids[keep], -(s[keep] + 0.0)))]
    return ids[o], s[o]


def same_range(got, ids, s, thr):
    wi, ws = range_want(ids, s, thr)
    assert [i for i, _ in got] == wi.tolist()
    assert np.array_equal(bits([v for _, v in got]), bits(ws))


@pytest.mark.parametrize("name", NAMES)
def test_range(name):
    """Section 5.14: a NaN score never qualifies, -inf returns every item whose score is a number."""
    asp, fx, gp, aspace, gl, V, ref = index(name)
    n = fx["X"].shape[0]
    inf = float("inf")
    for ids, handle in ((np.arange(n), None), (subsets(name)["one-block mix"], aspace.subset(subsets(name)["one-block mix"]))):
        for j, tau in ((0, 0.62), (5, 0.0)):
            s = aspace.score_items(V[j], gl, tau, ids)
            term = float(s[np.flatnonzero(np.isin(ids, fx["lam_rows"]))[0]])   # the lambda term of a NaN row
            for thr in (-inf, term, float(np.nanmedian(s)), inf):
                got = aspace.search_range(V[j], gl, tau, thr, subset=handle)
                same_range(got, ids, s, thr)
                assert aspace.count_range(V[j], gl, tau, thr, subset=handle) == len(got)
            got = aspace.search_range(V[j], gl, tau, -inf, subset=handle)
            assert sorted(i for i, _ in got) == ids[~np.isnan(s)].tolist() and 0 < len(got) < len(ids)
            assert set(fx["lam_rows"]) & set(ids.tolist()) <= set(i for i, _ in aspace.search_range(V[j], gl, tau, term, subset=handle))
        Q = V[:5]
        S = aspace.score_items_batch(Q, gl, 0.62, ids)
        thr = [-inf, inf, float(S[2][np.flatnonzero(np.isin(ids, fx["lam_rows"]))[0]]), float(np.nanmedian(S[3])), 2.0]
        got = aspace.search_range_batch(Q, gl, 0.62, thr, subset=handle)
        for i in range(5):
            same_range(got[i], ids, S[i], thr[i])
        assert aspace.count_range_batch(Q, gl, 0.62, thr, subset=handle).tolist() == [len(g) for g in got]


OVERFLOW = (-0.2, (1.7e308, -1.7e308, 1.0))   # tau and weights: a score above 1.0575 times 1.7e308 is inf; at this tau some are, some are not


@pytest.mark.parametrize("name", NAMES)
def test_fused(name):
    """S13: under max a NaN never displaces a number and F is NaN only if every term is; under sum a NaN term poisons F, and
    inf - inf arises from overflowing weights."""
    asp, fx, gp, aspace, gl, V, ref = index(name)
    n, topk = fx["X"].shape[0], gp["topk"]
    Q = V[:3]   # the overflow rows' queries: row huge[h] is a NaN term of vector h alone -- the first, the middle, the last
    mix = subsets(name)["one-block mix"]
    wide = subsets(name).get("threshold inside the NaN run", mix)
    for ids, handle in ((np.arange(n), None), (wide, aspace.subset(wide))):
        for tau, w in ((0.62, None), (0.62, (0.5, -0.25, 2.0)), OVERFLOW):
            S = aspace.score_items_batch(Q, gl, tau, ids)
            for mode in ("sum", "max"):
                with np.errstate(all="ignore"):
                    F = fused_ref.fuse(S, np.full(3, 1.0 / 3.0) if w is None else w, mode)
                same_scores(aspace.score_fused(Q, gl, tau, ids, weights=w, mode=mode), F)
                same_hits(aspace.search_fused(Q, gl, tau, weights=w, mode=mode, subset=handle), ids, F, min(topk, len(ids)))
                allnan = np.isnan(S).all(axis=0)
                assert allnan.any() and np.array_equal(np.isnan(F), allnan if mode == "max" else np.isnan(F))
                if mode == "max":
                    assert not np.isnan(F[np.isin(ids, fx["huge"])]).any()
                elif w is not OVERFLOW[1]:
                    assert np.array_equal(np.isnan(F), np.isnan(S).any(axis=0))
                if w is OVERFLOW[1] and mode == "sum" and handle is None:
                    assert (F == np.inf).any() and (F == -np.inf).any() and np.isfinite(F).any() and (np.isnan(F) & ~np.isnan(S).any(axis=0)).any()


def grouped_labels(fx):
    """name -> labels: the inf run is group 0 (no member: it never appears), group 1 is half inf (10 numbers, 10 NaN)."""
    n = fx["X"].shape[0]
    r0, r1 = fx["rows"]["run"][0], fx["rows"]["run"][-1] + 1
    crafted = 10 + np.arange(n) // 7
    crafted[r0:r1] = 0
    crafted[r0 - 10:r0 + 10] = 1
    return {"i // 7": np.arange(n) // 7, "one for all": np.full(n, 42), "singletons": np.arange(n), "crafted": crafted}


def same_groups(got, want):
    flat = lambda r: [(int(l), [(int(i), int(np.float64(s).view(np.uint64))) for i, s in mem]) for l, mem in r]
    assert flat(got) == flat(want)
    assert all(s == s for _, mem in got for _, s in mem)   # a NaN item is never a member


@pytest.mark.parametrize("name", NAMES)
def test_grouped(name):
    """S14: an item whose score is NaN belongs to no answer, a group of such items does not exist."""
    asp, fx, gp, aspace, gl, V, ref = index(name)
    n = fx["X"].shape[0]
    mix = subsets(name)["one-block mix"]
    r0 = fx["rows"]["run"][0]
    tail = np.arange(r0 - 10, n)   # the crafted groups and everything behind them
    Q = V[:3]
    for lname, labels in grouped_labels(fx).items():
        grp = aspace.groups(labels)
        for ids, handle in ((np.arange(n), None), (mix, aspace.subset(mix)), (tail, aspace.subset(tail))):
            s = aspace.score_items(V[0], gl, 0.62, ids)
            S = aspace.score_items_batch(Q, gl, 0.62, ids)
            for ng, pg in ((5, 1), (3, 3), (1024, 16)):
                got = aspace.search_grouped(V[0], gl, 0.62, grp, ng, pg, subset=handle)
                same_groups(got, grouped_ref.grouped(ids, labels[ids], s, ng, pg))
                res = aspace.search_batch_grouped(Q, gl, 0.62, grp, ng, pg, subset=handle)
                for i in range(3):
                    same_groups(res[i], grouped_ref.grouped(ids, labels[ids], S[i], ng, pg))
                if lname == "crafted" and handle is not None and ids is tail:
                    assert 0 not in [l for l, _ in got]
                    if ng == 1024:   # per_group = 16 stops at the numbers
                        assert [len(mem) for l, mem in got if l == 1] == [10] and 1 in [l for l, _ in got]
                if lname == "one for all" and ng == 1024:
                    assert len(got) == 1 and len(got[0][1]) == min(16, int((~np.isnan(s)).sum()))
    labels = grouped_labels(fx)["crafted"]
    S = aspace.score_items_batch(V[:65], gl, 0.62, np.arange(n))
    res = aspace.search_batch_grouped(V[:65], gl, 0.62, labels, 7, 3)
    for i in range(65):
        same_groups(res[i], grouped_ref.grouped(np.arange(n), labels, S[i], 7, 3))


@pytest.mark.parametrize("name", NAMES)
def test_diverse(name):
    """S12 over pools that hold NaN scores (margin -inf), rows whose cosine with a picked row is NaN, and zero rows (cosine 0)."""
    asp, fx, gp, aspace, gl, V, ref = index(name)
    X, d = fx["X"], fx["X"].shape[1]
    with np.errstate(all="ignore"):
        n64 = np.einsum("ij,ij->i", X, X)
    rng = np.random.default_rng(13)
    good = np.setdiff1d(np.arange(X.shape[0]), fx["bad"])
    S = np.sort(np.concatenate([fx["rows"]["pinf"], fx["rows"]["run"][:3], fx["lam_rows"], fx["huge"], fx["rows"]["inf_at_zcol"], rng.choice(good, 30, replace=False)]).astype(np.int64))
    sub = aspace.subset(S)
    assert len(S) <= gp["topk"]   # the pool is the whole subset
    tol = diverse_ref.tol_for(d)

    def verify(res, pool, delta):
        ids, s = [i for i, _ in pool], np.array([v for _, v in pool])
        assert len(res) == len(pool) == len(S) and np.isnan(s).any() and sorted(ids) == S.tolist()
        assert res[0][0] == ids[0] and len(set(i for i, _, _ in res)) == len(res)
        pos = {i: p for p, i in enumerate(ids)}
        same_scores([v for _, v, _ in res], s[[pos[i] for i, _, _ in res]])
        with np.errstate(all="ignore"):
            diverse_ref.check_steps(res, X, n64, ids, s, delta, tol)
            picks, margins, gaps = diverse_ref.mmr_path(X, n64, ids, s, len(ids), delta)
        for t, p in enumerate(picks):   # the path itself, as far as it is unambiguous; ties at -inf go to the earlier pool entry
            if t > 0 and margins[t] > -diverse_ref.INF and gaps[t] < 100 * tol:
                break
            assert res[t][0] == ids[p], (t, res[t], ids[p])
        numbers = int((~np.isnan(s)).sum())
        assert all(v == v for _, v, _ in res[:numbers]) and all(m == -diverse_ref.INF for _, _, m in res[numbers:])

    for delta in (0.0, 0.5, 1.0):
        for j in (0, 5):
            verify(aspace.search_diverse(V[j], gl, 0.62, len(S), delta, subset=sub, with_margins=True), aspace.search_subset(V[j], gl, 0.62, sub), delta)
        pools = aspace.search_batch_subset(V[:3], gl, 0.62, sub)
        for res, pool in zip(aspace.search_batch_diverse(V[:3], gl, 0.62, len(S), delta, subset=sub, with_margins=True), pools):
            verify(res, pool, delta)
