"""GPU: greedy k-means++ seeding -- ArrowSpace.kmeans_seed and kmeans(init="k-means++") against
tests/kmeans_seed_ref.py.  The distance kernel's tile and the potential's segment are 256 rows, its K stage 32 columns (16 on fp64
rows) and its candidate tile 16 wide, so n is one below, at and above the segment and in a third one, d below, above and far from a
multiple of the stage, L one, a few, the full tile and the default: a sparse pairing (CASES), not the product.  Integer items are
stored as fp32 rows, the Gaussian ones as fp64 rows: both instantiations run."""
import numpy as np
import pytest

import kmeans_ref as kr
import kmeans_seed_ref as ksr
from conftest import calibrate_eps

pytestmark = pytest.mark.gpu

CASES = [(255, 16, 1, 1), (255, 16, 5, 3), (256, 33, 2, 16), (256, 33, 17, None), (257, 70, 5, 1), (257, 70, 17, 16), (513, 16, 17, 3),
         (513, 70, 5, None), (513, 33, 2, 1)]
_built = {}


def space(kind, n=0, d=0):
    """One index per (kind, shape) for the whole module -> (ArrowSpace, the items it stores)."""
    import pyarrowspace_amd as asp
    key = (kind, n, d)
    if key not in _built:
        X = {"int": lambda: kr.integer_items(n, d, n + d), "gauss": lambda: kr.gaussian_items(n, d, n + d), "rep": ksr.repeated_items,
             "nan": lambda: kr.nan_case()[0], "mix": kr.mixture}[kind]()
        gp = {"eps": calibrate_eps(np.nan_to_num(X), 4, "l2") or 1.0, "k": 4, "topk": 4, "p": 2.0, "sigma": None, "metric": "l2", "kernel": "gaussian"}
        _built[key] = (asp.ArrowSpaceBuilder.build(gp, X), X)
    return _built[key][0][0], _built[key][1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_pinned(aspace, X, k, L, seed):
    Lr = L or ksr.default_trials(k)
    want = ksr.seed(X, k, Lr, seed)
    ids, info = aspace.kmeans_seed(k, seed=seed, trials=L, with_info=True)
    assert (ids.dtype, info["phi"].dtype, info["chosen"].dtype, info["candidates"].shape) == (np.int64, np.float64, np.int32, (k - 1, Lr))
    assert np.array_equal(ids, want["ids"]) and np.array_equal(bits(info["phi"]), bits(want["phi"]))
    assert np.array_equal(info["candidates"], want["candidates"]) and np.array_equal(info["chosen"], want["chosen"])
    assert info["degenerate"] == want["degenerate"] and np.array_equal(aspace.kmeans_seed(k, seed=seed, trials=L), ids)
    return want


@pytest.mark.parametrize("n,d,k,L", CASES)
def test_pinned_on_integer_items(n, d, k, L):
    aspace, X = space("int", n, d)
    want = check_pinned(aspace, X, k, L, n + k)
    assert want["degenerate"] == 0 and len(set(want["ids"].tolist())) == k


def test_the_fill_rule_takes_over_when_the_distinct_rows_run_out():
    aspace, X = space("rep")
    want = check_pinned(aspace, X, 7, 3, 2)
    assert want["degenerate"] == 2 and want["phi"][4:].tolist() == [0.0] * 3 and want["chosen"][4:].tolist() == [-1, -1]
    assert want["ids"][5:].tolist() == sorted(set(range(257)) - set(want["ids"][:5].tolist()))[:2]


@pytest.mark.parametrize("n,d,k,L", CASES)
def test_bounded_on_fp64_items(n, d, k, L):
    import pyarrowspace_amd as asp
    aspace, X = space("gauss", n, d)
    ids, info = aspace.kmeans_seed(k, seed=n + k, trials=L, with_info=True)
    ksr.check_replay(X, k, L or ksr.default_trials(k), n + k, ids, info)
    try:
        for cap in (1, 2):   # the later trips of the stride loop: same bits
            assert asp._L.as_set_tuning(b"kmeans_seed_grid_cap", cap) == 0
            again, ainfo = aspace.kmeans_seed(k, seed=n + k, trials=L, with_info=True)
            assert np.array_equal(again, ids) and np.array_equal(bits(ainfo["phi"]), bits(info["phi"])), cap
    finally:
        assert asp._L.as_set_tuning(b"kmeans_seed_grid_cap", 0) == 0


def test_a_row_with_a_nan_is_never_a_candidate():
    aspace, X = space("nan", 129, 33)
    live = np.arange(129) != kr.NAN_ROW
    k, L, seed = 9, 3, 4
    assert ksr.draws(129, k, L, seed)[0] != kr.NAN_ROW
    ids, info = aspace.kmeans_seed(k, seed=seed, trials=L, with_info=True)
    assert np.isfinite(info["phi"]).all()
    ksr.check_replay(X, k, L, seed, ids, info, live)


def test_kmeans_takes_the_seeding_by_name_and_the_host_waits_once_a_call():
    aspace, X = space("mix")
    c0 = aspace.kmeans_seed_counters()
    ids = aspace.kmeans_seed(6, seed=3)
    c1 = aspace.kmeans_seed_counters()
    assert [c1[key] - c0[key] for key in ("calls", "steps", "distance launches", "pick launches", "host waits")] == [1, 5, 6, 6, 1]
    ksr.check_replay(X, 6, ksr.default_trials(6), 3, *aspace.kmeans_seed(6, seed=3, with_info=True))
    cent, labels, info = aspace.kmeans(6, init="k-means++", seed=3, with_info=True)
    wcent, wlabels, winfo = aspace.kmeans(6, init=ids, seed=3, with_info=True)
    assert np.array_equal(labels, wlabels) and np.array_equal(bits(cent), bits(wcent))
    assert all(np.array_equal(info[key], winfo[key]) for key in winfo) and info["converged"]
    c2 = aspace.kmeans_seed_counters()
    assert (c2["calls"] - c1["calls"], c2["host waits"] - c1["host waits"]) == (2, 2)
    with pytest.raises(ValueError, match="init"):
        aspace.kmeans(6, init="k-means")
