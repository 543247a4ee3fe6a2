"""CPU: what `ArrowSpace.kmeans_seed` refuses before the library is reached, its default number of trials, the strings `kmeans`
accepts as `init`, and the bound C entries."""
import inspect

import numpy as np
import pytest

import kmeans_seed_ref as ksr


def handleless(n=10, d=4):
    """An ArrowSpace without a handle: everything up to the first use of the library runs."""
    import pyarrowspace_amd as asp
    cls = type("Handleless", (asp.ArrowSpace,), {"nitems": n, "nfeatures": d, "_h": None})
    return object.__new__(cls)


def test_refusals_and_the_default_trials():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    par = A._kmeans_seed_params
    assert [par(k, None, 10 ** 6)[1] for k in (1, 8, 1024, 4096)] == [2, 4, 8, 10] == [ksr.default_trials(k) for k in (1, 8, 1024, 4096)]
    assert par(np.int64(10), np.int32(16), 10) == (10, 16) and par(1, 1, 1) == (1, 1)
    sp = handleless()
    for k in (0, 11, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="k must"):
            sp.kmeans_seed(k)
    with pytest.raises(ValueError, match="k must"):
        par(4097, None, 10 ** 6)
    for trials in (0, 17, 2.0, True, "2"):
        with pytest.raises(ValueError, match="trials must"):
            sp.kmeans_seed(3, trials=trials)
    with pytest.raises(ValueError, match="row-sharded"):
        par(3, None, 10, row_offset=200)
    with pytest.raises(ValueError, match="init"):      # only the exact string names the seeding
        sp.kmeans(3, init="k-means")
    with pytest.raises(ValueError, match="init"):
        A._kmeans_init_ids(3, "k-means++", 0, 10)


def test_signatures_and_bound_entries():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    sig = inspect.signature(A.kmeans_seed)
    assert list(sig.parameters) == ["self", "k", "seed", "trials", "with_info"]
    assert [sig.parameters[p].default for p in ("seed", "trials", "with_info")] == [0, None, False] and callable(A.kmeans_seed_counters)
    out = np.zeros(8, dtype=np.int64)
    L, p, EINVAL = asp._L, out.ctypes.data, asp._lib.AS_EINVAL
    assert L.as_kmeans_seed(None, 1, 0, p, 1, p, p, p, p, p) == EINVAL and "as_kmeans_seed: null argument" in asp._lib.last_error()
    assert L.as_kmeans_seed_counters(None, p, 5) == EINVAL and L.as_kmeans_seed_kernel_us(None, 0) == 0.0
    assert L.as_set_tuning(b"kmeans_seed_grid_cap", 0) == 0

