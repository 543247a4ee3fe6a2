"""CPU: the surface of `ArrowSpace.assign_cosine`, `kmeans_spherical` and their debug forms: signatures, docstrings under both module
names, the C entries' null-argument returns and the refusals that need no handle."""
import inspect

import numpy as np
import pytest


def test_signatures_docstrings_and_bound_entries():
    import arrowspace
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    assert arrowspace.ArrowSpace is A
    sig = inspect.signature(A.assign_cosine)
    assert list(sig.parameters) == ["self", "centroids", "with_cos"] and sig.parameters["with_cos"].default is False
    assert inspect.signature(A.kmeans_spherical) == inspect.signature(A.kmeans)
    assert [list(inspect.signature(f).parameters) for f in (A._kmeans_spherical_update, A._kmeans_row_scales)] == [["self", "labels", "centroids"], ["self"]]
    for mod in (asp, arrowspace):
        for name in ("assign_cosine", "kmeans_spherical", "kmeans_spherical_counters"):
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:"), name
    out = np.zeros(16, dtype=np.int64)
    L, p, EINVAL, err = asp._L, out.ctypes.data, asp._lib.AS_EINVAL, asp._lib.last_error
    assert L.as_kmeans_cos_assign(None, p, 1, 1, p, p) == EINVAL and "as_kmeans_cos_assign: null argument" in err()
    assert L.as_kmeans_spherical(None, p, 1, 1, 1, p, p, p, p, p) == EINVAL and "as_kmeans_spherical: null argument" in err()
    assert L.as_kmeans_spherical_update(None, p, p, 1, 1, p) == EINVAL and "as_kmeans_spherical_update: null argument" in err()
    assert L.as_kmeans_spherical_scales(None, p) == EINVAL and "as_kmeans_spherical_scales: null argument" in err()
    assert L.as_kmeans_spherical_counters(None, p, 8) == EINVAL and L.as_kmeans_spherical_kernel_us(None, 0) == 0.0


@pytest.mark.parametrize("rows", [[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0], [1e200, 1e200, 0.0]], [[1e-170, 1e-170, 0.0]]])
def test_a_centroid_without_a_direction_is_refused_without_a_handle(rows):
    import pyarrowspace_amd as asp
    c = asp.ArrowSpace._kmeans_centroids(rows, 3)
    with pytest.raises(ValueError, match="has no direction"):
        asp.ArrowSpace._kmeans_directions(c)
    assert asp.ArrowSpace._kmeans_directions(np.array([[3.0, 4.0, 0.0]]), "init").shape == (1, 3)
