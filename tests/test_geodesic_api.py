"""CPU: what `ArrowSpace.shortest_paths`, `score_geodesic`, `search_geodesic` and `search_batch_geodesic` refuse before a handle is
touched (the refusals that need a graph are in tests/test_gpu_geodesic.py)."""
import numpy as np
import pytest


def test_python_validators_run_before_a_handle_is_touched():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    sources, cutoff, seeds = A._geodesic_sources, A._geodesic_cutoff, A._geodesic_seeds
    ids, offs, starts = sources([3, ([1, 2], [0.5, -0.0]), ([], [])], 10)
    assert ids.tolist() == [3, 1, 2] and offs.tolist() == [0.0, 0.5, 0.0] and starts.tolist() == [0, 1, 3, 3]
    assert sources([], 10)[2].tolist() == [0]
    for bad in ([10], [-1], [([0, 10], [0.0, 0.0])], [([1, 1], [0.0, 1.0])]):          # an id outside [0, nitems), a repeated id
        with pytest.raises(ValueError):
            sources(bad, 10)
    for bad in ([([1], [-1e-300])], [([1], [np.nan])], [([1], [np.inf])], [([1, 2], [0.0])]):   # a negative, NaN or infinite offset
        with pytest.raises(ValueError):
            sources(bad, 10)
    for bad in ([1.5], [True], [([1.0], [0.0])]):                                       # an id that is no integer
        with pytest.raises(TypeError):
            sources(bad, 10)
    for bad in (3, "12", None):                                                         # not a sequence of sources
        with pytest.raises((ValueError, TypeError)):
            sources(bad, 10)
    assert cutoff(None) is None and cutoff(2).value == 2.0 and cutoff(np.inf).value == np.inf and cutoff(-1.0).value == -1.0
    for bad in (float("nan"), np.float64("nan"), "1.0", True, [1.0]):
        with pytest.raises(ValueError, match="cutoff"):
            cutoff(bad)
    assert seeds(1, 8) == 1 and seeds(np.int64(8), 8) == 8
    for bad in (0, 9, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="seeds"):
            seeds(bad, 8)
    for name in ("shortest_paths", "score_geodesic", "search_geodesic", "search_batch_geodesic", "geodesic_counters"):
        assert callable(getattr(A, name))
    with pytest.raises(TypeError):
        A.shortest_paths(object.__new__(A), None, [0])   # (the graph is checked before the handle is used)
    assert asp._L.as_geodesic_seeds(None, None, None, None, None, 0, None, None, 0, None, None) == asp._lib.AS_EINVAL
