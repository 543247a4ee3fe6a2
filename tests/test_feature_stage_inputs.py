"""CPU: the hand-built inputs of tests/test_gpu_feature_stage.py (tests/feature_stage_ref.py) have the properties they are
named for, and each F3 fixture can see the error it is aimed at: the expected CSR -- indices and values -- changes under a
deliberately wrong F3 written here.  Union symmetrisation can hide a wrong directed list behind the reverse edge; a fixture
whose CSR does not move under its variant proves nothing and would have to be redesigned."""
import numpy as np
import pytest

import feature_stage_ref as fx
from oracle import oracle_np


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _prm(gp):
    return oracle_np.resolve_params(gp)


# ------------------------------------------------------------------------------------------------ wrong F3s
def f3_lists(key, ek, k, variant=None):
    """SPEC F3 (b != a, key <= eps key, order (key asc, b asc), first k), or one of four wrong variants of it."""
    D = key.shape[0]
    out = []
    for a in range(D):
        ok = key[a] < ek if variant == "strict_eps" else key[a] <= ek
        if variant != "self_admitted":
            ok[a] = False
        idx = np.nonzero(ok)[0]
        tie = -idx if variant == "descending_ties" else idx
        idx = idx[np.lexsort((tie, key[a][idx]))]
        out.append(idx[: k - 1 if variant == "cut_short" else k])
    return out


def csr_of(gram, gp, variant=None):
    """(indptr, indices, values) of L = D - W off the diagonal from F3's lists, the oracle's F4 / F5."""
    prm = _prm(gp)
    key = fx.keys_of(gram, prm)
    dist = np.sqrt(key) if prm["metric"] == oracle_np.METRIC_L2 else key
    lists = f3_lists(key, oracle_np._eps_key(prm["eps"], prm["metric"]), prm["k"], variant)
    D = key.shape[0]
    adj = [set() for _ in range(D)]
    for a, js in enumerate(lists):
        for b in js:
            adj[a].add(int(b))
            adj[int(b)].add(a)
    indptr = np.cumsum([0] + [len(s) for s in adj])
    rows = np.repeat(np.arange(D), np.diff(indptr))
    cols = np.array([b for s in adj for b in sorted(s)], dtype=np.int64)
    d = dist[np.minimum(rows, cols), np.maximum(rows, cols)] if len(cols) else np.zeros(0)
    w = oracle_np._edge_weight(d, prm["sigma"], prm["p"], prm["kernel"]) if len(cols) else d
    return indptr, cols, -w


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(fx.GRAM_FIXTURES))
def test_the_right_f3_written_here_is_the_oracles(name):
    gram, gp = fx.GRAM_FIXTURES[name]()
    assert np.array_equal(gram, gram.T)
    ref = fx.expected_graph(name)
    ip, ix, v = csr_of(gram, gp)
    assert np.array_equal(ip, ref["indptr"]) and np.array_equal(ix, ref["indices"]) and np.array_equal(_bits(v), _bits(ref["lap"]))


@pytest.mark.parametrize("name,variant", [("tie", "descending_ties"), ("tie", "cut_short"), ("tie", "self_admitted"),
                                          ("eps", "strict_eps"), ("cosine_eps1", "strict_eps"), ("cosine_eps1", "descending_ties"),
                                          ("cosine_eps1", "cut_short"), ("d2", "cut_short"), ("d2", "self_admitted"),
                                          ("kclamp", "self_admitted"), ("l2_clamp", "self_admitted")])
def test_fixture_sees_its_wrong_f3(name, variant):
    gram, gp = fx.GRAM_FIXTURES[name]()
    right, wrong = csr_of(gram, gp), csr_of(gram, gp, variant)
    assert not (np.array_equal(right[1], wrong[1]) and np.array_equal(right[0], wrong[0])), "topology unchanged"
    assert not _same(right, wrong)


# ------------------------------------------------------------------------------------------------ named properties
def test_tie_run_contains_the_cut_and_straddles_column_256():
    gram, gp = fx.tie_fixture()
    prm = _prm(gp)
    key = fx.keys_of(gram, prm)[fx.TIE_HUB]
    assert np.array_equal(key, np.round(key))                      # integer keys: equal keys are equal bits
    ek = oracle_np._eps_key(prm["eps"], prm["metric"])
    idx = np.array([b for b in range(fx.TIE_D) if b != fx.TIE_HUB and key[b] <= ek])
    idx = idx[np.lexsort((idx, key[idx]))]
    k = prm["k"]
    kth = key[idx[k - 1]]
    run = np.nonzero(key[idx] == kth)[0]
    assert len(run) >= 6 and run[0] < k - 1 and run[-1] > k        # members on both sides of the cut
    assert tuple(sorted(idx[run])) == fx.TIE_MEMBERS
    taken, left = idx[run[0] : k], idx[k : run[-1] + 1]
    # the block's first 256-thread trip handles columns < 256: tied columns of both trips are taken, and left out
    assert (taken < 256).any() and (taken >= 256).any() and (left >= 256).any()
    ref = fx.expected_graph("tie")
    assert ref["knn"][fx.TIE_HUB].tolist() == idx[:k].tolist()
    for t in fx.TIE_MEMBERS:                                       # no reverse edge hides the hub's choice
        assert fx.TIE_HUB not in ref["knn"][t] and len(ref["knn"][t]) == k
    # fewer than k passers, and none
    assert [len(ref["knn"][c]) for c in fx.TIE_PAIR] == [1, 1]
    lonely = [c for c in range(fx.TIE_D) if len(ref["knn"][c]) == 0]
    assert len(lonely) > 100 and min(lonely) < 256 < max(lonely)
    assert 0 < len(ref["knn"][11]) and len(ref["knn"][11]) == k


def test_shifted_tie_fixture_is_a_monotone_relabelling():
    gram, gp = fx.tie_fixture()
    big, gp2, keep = fx.tie_fixture_shifted()
    assert gp2 == gp and np.all(np.diff(keep) > 0) and np.array_equal(big[np.ix_(keep, keep)], gram)
    a, b = fx.expected_graph("tie"), oracle_np.feature_graph_from_gram(big, _prm(gp))
    assert np.array_equal(keep[a["indices"]], b["indices"]) and np.array_equal(_bits(a["lap"]), _bits(b["lap"]))
    assert np.array_equal(_bits(a["deg"]), _bits(b["deg"][keep]))
    assert (keep[np.array(fx.TIE_MEMBERS)] >= 256).sum() == (np.array(fx.TIE_MEMBERS) >= 256).sum() + 1


def test_eps_fixture_sits_on_the_line():
    gram, gp = fx.eps_fixture()
    prm = _prm(gp)
    ek = oracle_np._eps_key(prm["eps"], prm["metric"])
    key = fx.keys_of(gram, prm)
    assert _bits(key[0, 1]) == _bits(ek) and _bits(key[0, 2]) == _bits(ek) + 1
    ref = fx.expected_graph("eps")
    assert ref["knn"][0].tolist() == [3, 1] and ref["knn"][1].tolist() == [0] and ref["knn"][2].tolist() == []


def test_cosine_and_clamp_fixtures():
    g, gp = fx.cosine_fixture(1.0)
    m = np.diagonal(g)
    key = fx.keys_of(g, _prm(gp))
    assert g[0, 2] > np.sqrt(m[0] * m[2]) and g[0, 2] / np.sqrt(m[0] * m[2]) > 1.0 and key[0, 2] == 0.0 and key[0, 1] == 0.0
    assert m[5] == 0.0 and np.all(key[5, np.arange(8) != 5] == 1.0)
    assert np.all(g[4, [0, 1, 2, 3, 6, 7]] < 0) and np.all(key[4, np.arange(8) != 4] == 1.0)
    r1, r09 = fx.expected_graph("cosine_eps1"), fx.expected_graph("cosine_eps09")
    assert r1["knn"][0].tolist() == [1, 2] and r1["knn"][3].tolist() == [0, 1]
    assert r1["knn"][4].tolist() == [0, 1] and r1["knn"][5].tolist() == [0, 1]
    assert r09["knn"][4].tolist() == [] and r09["knn"][5].tolist() == [] and r09["knn"][0].tolist() == [1, 2]
    g, gp = fx.l2_clamp_fixture()
    assert g[0, 0] + g[1, 1] - 2.0 * g[0, 1] < 0.0 and _bits(g[0, 1]) == _bits(g[0, 0]) + 1
    ref = fx.expected_graph("l2_clamp")
    e = np.nonzero((np.repeat(np.arange(3), np.diff(ref["indptr"])) == 0) & (ref["indices"] == 1))[0]
    assert len(e) == 1 and ref["dist"][e[0]] == 0.0 and ref["lap"][e[0]] == -1.0
    # k >= D - 1; D = 1, 2
    assert [len(l) for l in fx.expected_graph("kclamp")["knn"]] == [5] * 6
    assert len(fx.expected_graph("d1")["indices"]) == 0 and fx.expected_graph("d2")["indices"].tolist() == [1, 0]


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_storage_of_the_items(storage):
    arrays = [fx.gram_items(fx.GRAM_N, d, storage) for d in fx.GRAM_DS] + [fx.path_vectors(storage)[0]]
    for X in arrays:
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X) == (storage == "f32")
    if storage == "f32":
        arrays = [fx.gram_items(*fx.GRAM_BIG, "f32"), fx.wide_fixture(50, 2401)[0], fx.wide_fixture(1101, 4801)[0]]
    else:
        arrays = [fx.range_fixture()[0], fx.wide_fixture(50, 3201)[0]] + [fx.scaled_base(*s)[0] for s in fx.SCALED_SHAPES]
    for X in arrays:
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X) == (storage == "f32")


def test_gram_items_are_exact_in_any_order():
    for storage in ("f32", "f64"):
        for d in fx.GRAM_DS:
            X = fx.gram_items(fx.GRAM_N, d, storage)
            assert np.array_equal(X, np.round(X))
            assert np.array_equal(sum(fx.int_gram_of(X, a, b) for a, b in fx.GRAM_SPLIT), fx.int_gram_of(X, 0, fx.GRAM_N))
            assert (np.abs(X) ** 2).sum(0).max() < 2 ** 53
    n, d = fx.GRAM_BIG
    assert n > 16384 and -(-n // 16384) == 2 and -(-(n - 7) // 16384) == 2      # nsplit = 2, whole and from row 7
    rps = -(-(-(-n // 2)) // 32) * 32
    assert 0 < n - rps < rps                                                   # the second split is the shorter one


def test_path_vectors_have_the_energies_they_are_named_for():
    gram, gp = fx.path_fixture()
    idx = oracle_np.feature_graph_from_gram(gram, _prm(gp))
    assert len(idx["ew"]) == 10 and len(set(idx["ew"].tolist())) == 1
    for storage in ("f32", "f64"):
        X, g_want = fx.path_vectors(storage)
        diff = X[:, idx["ea"]] - X[:, idx["eb"]]
        assert ((diff != 0).sum(1) == np.array([0, 0, 1, 1, 2, 2])).all()
        assert all(len(set(np.abs(r[r != 0]).tolist())) <= 1 for r in diff)
        E, G = oracle_np.feature_energy(idx, X)
        assert np.array_equal(G, g_want) and np.array_equal(E[:2], [0.0, 0.0]) and (E[2:] > 0).all()


def test_wide_rows_launch_shapes():
    """What as_feat.hip derives for the wide shapes on a 256-CU device: 3, 2 and 1 waves per block, and at 4801 features
    three trips of the stride loop whose last one ends in a lone row."""
    assert [fx.energy_launch(d, n, 256)[0] for n, d in fx.WIDE_SHAPES] == [3, 2, 1]
    assert [fx.energy_launch(d, 50, 256)[0] for d in (2400, 2401, 3200, 3201, 4800, 4801)] == [4, 3, 3, 2, 2, 1]
    waves, grid, trips, tail = fx.energy_launch(4801, 1101, 256)
    assert (waves, grid, trips, tail) == (1, 256, 3, 77) and tail % 2 == 1 and 256 * 2 < 1101
    assert 2 * 8 * 4801 > 64 * 1024                                 # feat_knn_kernel: more than 64 KiB of dynamic LDS
    for n, d in fx.WIDE_SHAPES:
        X, gram, gp = fx.wide_fixture(n, d)
        key = fx.keys_of(gram[:9, :9], _prm(gp))
        assert sorted(set(key[0, 1:3].tolist() + key[1, 2:4].tolist())) == [1.0, 1.5, 2.0]


@pytest.mark.parametrize("n,d,k", fx.SCALED_SHAPES)
def test_scaled_items_reach_the_ratio_pass_and_the_oracle_is_exact_there(n, d, k):
    X, gp = fx.scaled_base(n, d, k)
    base = fx.scaled_oracle(n, d, k, 0)
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    for s in fx.RATIO_SCALES + fx.CONTROL_SCALES:
        idx = fx.scaled_oracle(n, d, k, s)
        T = fx.edge_energy_sums(idx, np.ldexp(X, s))
        assert (T > 0).all()
        if s in fx.RATIO_SCALES:
            assert (T > 1e140).all() if s > 0 else (T < 1e-140).all()
        else:
            assert ((T > 1e-140) & (T < 1e140)).all()
        mm = np.outer(idx["m"], idx["m"])
        assert mm.min() >= tiny and mm.max() < huge and np.isfinite(mm).all()
        # power-of-two scaling is exact: the reference of the scaled index is the unscaled one, bit for bit
        assert np.array_equal(idx["indices"], base["indices"]) and idx["tau0"] == base["tau0"]
        for key in ("E", "G", "lambdas", "ew"):
            assert np.array_equal(_bits(idx[key]), _bits(base[key])), (s, key)
