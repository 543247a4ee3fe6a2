"""CPU: what `ArrowSpace.components` and `components_sweep` refuse before a handle is touched (the refusals that need a graph -- a
feature-mode index, a graph of another space's size -- are in tests/test_gpu_components.py), the bound C entries, and the reference
of tests/components_ref.py on small hand-made graphs whose answers can be read off."""
import inspect

import numpy as np
import pytest

import components_ref as cr


def test_python_validators_run_before_a_handle_is_touched():
    import pyarrowspace_amd as asp
    A = asp.ArrowSpace
    check = A._components_thresholds
    assert check(0.5, single=True).tolist() == [0.5] and check(np.float32(2.0), single=True).dtype == np.float64
    assert check(3, single=True).tolist() == [3.0] and check(np.int64(3), single=True).tolist() == [3.0]
    assert check(float("inf"), single=True).tolist() == [np.inf] and check(-np.inf, single=True).tolist() == [-np.inf]
    assert check([2.0, 1.0, 2.0, -np.inf, np.inf]).tolist() == [2.0, 1.0, 2.0, -np.inf, np.inf]   # any order, duplicates kept
    assert check(np.linspace(0.0, 1.0, 64)).shape == (64,) and check((1,)).tolist() == [1.0]
    for bad in (float("nan"), np.nan, np.float64("nan")):
        with pytest.raises(ValueError, match="NaN"):
            check(bad, single=True)
        with pytest.raises(ValueError, match="NaN"):
            check([1.0, bad, 2.0])
    for bad in ("1.0", None, [1.0], True, np.True_, 1j, object()):   # a non-numeric threshold
        with pytest.raises(ValueError, match="max_dist"):
            check(bad, single=True)
    for bad in ([1.0, "2.0"], [None], [True], ["a"], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="max_dists"):
            check(bad)
    for bad in ([], np.zeros(0), [1.0] * 65, np.zeros(65)):         # T = 0 and T = 65
        with pytest.raises(ValueError, match="1 to 64"):
            check(bad)
    for bad in (1.0, "abc", None, np.zeros((2, 2))):                # not a sequence
        with pytest.raises(ValueError, match="max_dists"):
            check(bad)


def test_signatures_and_bound_entries():
    import pyarrowspace_amd as asp
    A, G = asp.ArrowSpace, asp.GraphLaplacian
    sig = inspect.signature(A.components)
    assert list(sig.parameters) == ["self", "gl", "max_dist", "with_info"]
    assert [sig.parameters[k].default for k in ("max_dist", "with_info")] == [None, False]
    assert list(inspect.signature(A.components_sweep).parameters) == ["self", "gl", "max_dists"]
    assert A._COMPONENTS_KEYS == cr.KEYS + ("rounds",)
    for name in ("components", "components_sweep", "components_counters"):
        assert callable(getattr(A, name))
    assert callable(G.to_csr_dist) and callable(G.to_csr)
    with pytest.raises(TypeError):
        A.components(object.__new__(A), None)            # (the graph is checked before the handle is used)
    with pytest.raises(TypeError):
        A.components_sweep(object.__new__(A), None, [1.0])
    for sym in ("as_graph_components", "as_graph_components_sweep", "as_components_counters", "as_components_kernel_us", "as_graph_csr_dist"):
        assert getattr(asp._L, sym) is not None
    # null handles are refused by the C entries themselves
    out = np.zeros(6, dtype=np.int64)
    assert asp._L.as_graph_components(None, None, None, out.ctypes.data, out.ctypes.data) == asp._lib.AS_EINVAL
    assert asp._L.as_graph_components_sweep(None, None, out.ctypes.data, 1, out.ctypes.data) == asp._lib.AS_EINVAL
    assert asp._L.as_components_counters(None, out.ctypes.data, 5) == asp._lib.AS_EINVAL
    assert asp._L.as_graph_csr_dist(None, out.ctypes.data, out.ctypes.data, out.ctypes.data) == asp._lib.AS_EINVAL
    assert asp._L.as_components_kernel_us(None, 0) == 0.0


def small():
    """Seven items: 0 - 3 (dist 1), 3 - 5 (dist 2, stored one way round as both), 1 - 2 (dist NaN), 4 and 6 alone."""
    nbrs = [[3], [2], [], [5], [], [], []]
    dists = [[1.0], [np.nan], [], [2.0], [], [], []]
    return (7,) + cr.csr_of_lists(7, nbrs, dists)


def test_the_reference_on_a_graph_read_off_by_hand():
    g = small()
    assert g[1].tolist() == [0, 1, 2, 3, 5, 5, 6, 6] and g[2].tolist() == [3, 2, 1, 0, 5, 3]
    want = {None: [0, 1, 1, 0, 4, 0, 6], np.inf: [0, 1, 2, 0, 4, 0, 6], 2.0: [0, 1, 2, 0, 4, 0, 6], 1.5: [0, 1, 2, 0, 4, 5, 6],
            1.0: [0, 1, 2, 0, 4, 5, 6], 0.5: list(range(7)), -np.inf: list(range(7))}
    infos = {None: (4, 3, 0, 2, 6), np.inf: (5, 3, 0, 4, 4), 2.0: (5, 3, 0, 4, 4), 1.5: (6, 2, 0, 5, 2), 1.0: (6, 2, 0, 5, 2),
             0.5: (7, 1, 0, 7, 0), -np.inf: (7, 1, 0, 7, 0)}
    for t, lab in want.items():
        got = cr.components(*g, t)
        assert got.dtype == np.int32 and got.tolist() == lab, t
        assert tuple(cr.info(got, *g[1:], t)[k] for k in cr.KEYS) == infos[t], t
        sync, rounds = cr.sync_rounds(*g, t)
        assert sync.tolist() == lab and rounds == (0 if t in (0.5, -np.inf) else 1), t
    # a warm start from a smaller threshold's labels ends in the same labels
    assert cr.sync_rounds(*g, None, parent=cr.components(*g, 1.0))[0].tolist() == want[None]
    assert cr.canonical(np.array([5, 9, 9, 5, 2, 5, 7])).tolist() == want[None]


def test_largest_label_is_the_smallest_label_of_the_largest_size():
    # two classes of three: {1, 2, 6} and {0, 4, 5}; 3 alone
    nbrs = [[4], [2], [6], [], [5], [], []]
    g = (7,) + cr.csr_of_lists(7, nbrs, [[1.0] * len(x) for x in nbrs])
    lab = cr.components(*g)
    assert lab.tolist() == [0, 1, 1, 3, 0, 0, 1]
    assert cr.info(lab, *g[1:]) == {"count": 3, "largest": 3, "largest_label": 0, "isolated": 1, "edges_kept": 8}
