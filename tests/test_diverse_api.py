"""CPU: the surface of diversified search -- ArrowSpace.search_diverse / search_batch_diverse / diverse_counters (also under the
reference module name), the C ABI symbols behind them and what they refuse before a GPU is touched.  No compute call: the GPU
behaviour is tests/test_gpu_diverse.py's."""
import ctypes
import inspect
import os

import pytest

SYMBOLS = ("as_search_diverse", "as_search_diverse_batch", "as_diverse_counters", "as_diverse_kernel_us")


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_methods_exist_under_both_module_names(asp):
    import arrowspace
    assert arrowspace.ArrowSpace is asp.ArrowSpace
    for mod in (asp, arrowspace):
        for name in ("search_diverse", "search_batch_diverse", "diverse_counters"):
            assert callable(getattr(mod.ArrowSpace, name, None)), name
            assert getattr(mod.ArrowSpace, name).__doc__.startswith("Extension:")
    sig = inspect.signature(asp.ArrowSpace.search_diverse)
    assert list(sig.parameters) == ["self", "item", "gl", "tau", "n", "diversity", "subset", "with_margins"]
    assert sig.parameters["subset"].default is None and sig.parameters["with_margins"].default is False
    sig = inspect.signature(asp.ArrowSpace.search_batch_diverse)
    assert list(sig.parameters) == ["self", "items", "gl", "tau", "n", "diversity", "subset", "with_margins"]
    assert sig.parameters["subset"].default is None and sig.parameters["with_margins"].default is False


def test_library_exports_the_diverse_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in asp._lib.SYMBOLS, name
        assert f" {name}(" in hdr, name
    assert '"diverse_chunk"' in hdr and '"diverse_timing"' in hdr


def test_null_arguments_are_rejected_without_a_gpu(asp):
    L, EINVAL = asp._L, asp._lib.AS_EINVAL
    q = (ctypes.c_double * 8)()
    idx = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    sc = (ctypes.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    mg = (ctypes.c_double * 4)(5.0, 5.0, 5.0, 5.0)
    ln = (ctypes.c_int64 * 2)(9, 9)
    lq = (ctypes.c_double * 2)(3.0, 3.0)
    st = (ctypes.c_int32 * 2)(9, 9)
    assert L.as_search_diverse(None, None, q, 4, 0.5, 2, 0.5, None, idx, sc, mg, ln, lq) == EINVAL
    assert "as_search_diverse: null argument" in asp._lib.last_error()
    assert list(idx) == [7] * 4 and list(sc) == [5.0] * 4 and list(mg) == [5.0] * 4 and list(ln) == [9, 9] and list(lq) == [3.0, 3.0]
    assert L.as_search_diverse(None, None, None, 4, 0.5, 2, 0.5, None, None, None, None, None, None) == EINVAL
    assert L.as_search_diverse_batch(None, None, q, 2, 4, 0.5, 2, 0.5, None, idx, sc, mg, ln, lq, st) == EINVAL
    assert "as_search_diverse_batch: null argument" in asp._lib.last_error()
    assert list(idx) == [7] * 4 and list(ln) == [9, 9] and list(lq) == [3.0, 3.0] and list(st) == [9, 9]   # nothing was written
    assert L.as_search_diverse_batch(None, None, None, 0, 4, 0.5, 2, 0.5, None, None, None, None, None, None, None) == EINVAL
    out = (ctypes.c_int64 * 5)(1, 2, 3, 4, 5)
    assert L.as_diverse_counters(None, out, 5) == EINVAL and list(out) == [1, 2, 3, 4, 5]
    assert "as_diverse_counters: null argument" in asp._lib.last_error()
    assert L.as_diverse_kernel_us(None) == 0.0


def test_n_and_diversity_are_refused_without_a_gpu(asp):
    """The Python layer refuses them before it touches the handles: a space that holds no handle is enough."""
    space = object.__new__(asp.ArrowSpace)
    gl = object.__new__(asp.GraphLaplacian)
    import numpy as np
    q = np.zeros(4)
    Q = np.zeros((2, 4))
    for n, delta in ((0, 0.5), (-3, 0.5), (2, -0.1), (2, 1.1), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(ValueError, match="n must be|diversity must"):
            space.search_diverse(q, gl, 0.5, n, delta)
        with pytest.raises(ValueError, match="n must be|diversity must"):
            space.search_batch_diverse(Q, gl, 0.5, n, delta)
    for n in (2.0, "2", True, None):
        with pytest.raises(TypeError):
            space.search_diverse(q, gl, 0.5, n, 0.5)
    with pytest.raises(TypeError):
        space.search_diverse(q, None, 0.5, 2, 0.5)
    with pytest.raises(TypeError):
        space.search_batch_diverse(Q, None, 0.5, 2, 0.5)
    assert asp.ArrowSpace._diverse_params(np.int64(3), 1) == (3, 1.0)
    assert asp.ArrowSpace._diverse_params(1, 0.0) == (1, 0.0)


def test_chunk_and_timing_are_tuning_keys(asp):
    try:
        assert asp._L.as_set_tuning(b"diverse_chunk", 7) == 0
        assert asp._L.as_set_tuning(b"diverse_timing", 1) == 0
    finally:
        assert asp._L.as_set_tuning(b"diverse_chunk", 0) == 0
        assert asp._L.as_set_tuning(b"diverse_timing", 0) == 0
    assert asp._L.as_set_tuning(b"diverse_chunks", 4) == 1   # an unknown key
