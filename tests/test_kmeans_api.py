"""CPU: what `ArrowSpace.assign`, `kmeans` and `_kmeans_update` refuse before the library is reached, the ids of `init=None`,
and the bound C entries."""
import inspect

import numpy as np
import pytest


def test_python_validators_run_before_a_handle_is_touched():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    cent = A._kmeans_centroids
    got = cent(np.asfortranarray(np.ones((3, 5), dtype=np.float32)), 5)
    assert got.dtype == np.float64 and got.flags.c_contiguous and got.shape == (3, 5)
    assert cent(np.zeros((4096, 2)), 2).shape == (4096, 2) and cent([[1, 2]], 2).tolist() == [[1.0, 2.0]]
    for bad in (np.zeros(5), np.zeros((2, 3, 5)), np.zeros((3, 4)), np.zeros((0, 5)), np.zeros((4097, 5)), "abc", None, [["a"] * 5]):
        with pytest.raises(ValueError, match="centroids"):   # wrong rank, wrong width, k out of range, not numbers
            cent(bad, 5)
    for v in (np.nan, np.inf, -np.inf):
        C = np.zeros((3, 5))
        C[2, 4] = v
        with pytest.raises(ValueError, match="non-finite"):
            cent(C, 5)
    par = A._kmeans_params
    assert par(1, 1, 10) == (1, 1) and par(np.int64(10), np.int32(7), 10) == (10, 7) and par(4096, 25, 10 ** 6) == (4096, 25)
    for k, iters in ((0, 25), (11, 25), (4097, 25), (2.0, 25), (True, 25), ("3", 25), (3, 0), (3, -1), (3, 2.5), (3, None)):
        with pytest.raises(ValueError, match="k must|max_iters must"):
            par(k, iters, 10 if k != 4097 else 10 ** 6)
    ids = A._kmeans_init_ids
    assert ids(3, [4, 0, 9], 0, 10).tolist() == [4, 0, 9] and ids(2, np.array([1, 0], dtype=np.int32), 0, 10).dtype == np.int64
    for bad in ([1, 1, 2], [0, 1], [0, 1, 10], [-1, 0, 1], [0.0, 1.0, 2.0], [True, False, True], np.zeros((3, 1), dtype=np.int64), "abc"):
        with pytest.raises(ValueError, match="init"):
            ids(3, bad, 0, 10)
    # init=None: the ids of the stated generator call, in drawn order
    for seed, k, n in ((0, 5, 100), (7, 64, 1000), (123, 1, 3)):
        assert ids(k, None, seed, n).tolist() == np.random.default_rng(seed).choice(n, k, replace=False).tolist()


def test_signatures_and_bound_entries():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    sig = inspect.signature(A.kmeans)
    assert list(sig.parameters) == ["self", "k", "init", "seed", "max_iters", "with_info"]
    assert [sig.parameters[p].default for p in ("init", "seed", "max_iters", "with_info")] == [None, 0, 25, False]
    sig = inspect.signature(A.assign)
    assert list(sig.parameters) == ["self", "centroids", "with_dist"] and sig.parameters["with_dist"].default is False
    assert list(inspect.signature(A._kmeans_update).parameters) == ["self", "labels", "centroids"] and callable(A.kmeans_counters)
    out = np.zeros(8, dtype=np.int64)
    L, p, EINVAL = asp._L, out.ctypes.data, asp._lib.AS_EINVAL
    assert L.as_kmeans_assign(None, p, 1, 1, p, None) == EINVAL and "null argument" in asp._lib.last_error()
    assert L.as_kmeans(None, p, 1, 1, 1, p, p, p, p, p) == EINVAL and "as_kmeans: null argument" in asp._lib.last_error()
    assert L.as_kmeans_update(None, p, p, 1, 1, p) == EINVAL and L.as_kmeans_counters(None, p, 6) == EINVAL
    assert L.as_kmeans_kernel_us(None, 0) == 0.0
    for key in (b"kmeans_grid_cap", b"kmeans_timing"):
        assert L.as_set_tuning(key, 0) == 0
