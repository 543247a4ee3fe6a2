"""CPU: the surface of `ArrowSpace.kmeans_bounded` and `_kmeans_assign2`: signatures, the bound C entries' null-argument returns and
the tuning key."""
import inspect

import numpy as np


def test_signatures_and_bound_entries():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    sig = inspect.signature(A.kmeans_bounded)
    assert sig == inspect.signature(A.kmeans) and list(sig.parameters) == ["self", "k", "init", "seed", "max_iters", "with_info"]
    sig = inspect.signature(A._kmeans_assign2)
    assert list(sig.parameters) == ["self", "centroids", "ids"] and sig.parameters["ids"].default is None
    assert callable(A.kmeans_bounded_counters)
    out = np.zeros(16, dtype=np.int64)
    L, p, EINVAL = asp._L, out.ctypes.data, asp._lib.AS_EINVAL
    assert L.as_kmeans_bounded(None, p, 1, 1, 1, p, p, p, p, p, p) == EINVAL and "as_kmeans_bounded: null argument" in asp._lib.last_error()
    assert L.as_kmeans_assign2(None, p, 1, 1, None, 1, p, p, p) == EINVAL and "as_kmeans_assign2: null argument" in asp._lib.last_error()
    assert L.as_kmeans_bounded_counters(None, p, 9) == EINVAL and L.as_kmeans_bounded_kernel_us(None, 0) == 0.0
    assert L.as_set_tuning(b"kmeans_bounded_grid_cap", 0) == 0
