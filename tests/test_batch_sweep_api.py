"""CPU: the batched tau-sweep extension's surface -- ArrowSpace.search_batch_taus / batch_sweep_counters (also under the
reference module name) and the C ABI symbols behind them.  No compute call: the GPU behaviour is tests/test_gpu_batch_sweep.py's."""
import ctypes
import inspect
import os

import pytest


@pytest.fixture(scope="module")
def asp():
    import __graft_entry__ as g
    g.build()
    import pyarrowspace_amd
    return pyarrowspace_amd


def test_arrowspace_has_search_batch_taus_and_counters(asp):
    import arrowspace
    for cls in (asp.ArrowSpace, arrowspace.ArrowSpace):
        assert callable(getattr(cls, "search_batch_taus", None))
        assert callable(getattr(cls, "batch_sweep_counters", None))
        assert list(inspect.signature(cls.search_batch_taus).parameters) == ["self", "items", "gl", "taus"]
    assert asp.ArrowSpace.search_batch_taus.__doc__.startswith("Extension:")


def test_library_exports_the_batch_sweep_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    for name in ("as_search_batch_taus", "as_batch_sweep_counters"):
        assert hasattr(lib, name)
        assert name in asp._lib.SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    assert "as_status as_search_batch_taus(" in hdr and "as_status as_batch_sweep_counters(" in hdr


def test_batch_sweep_entry_points_reject_null_arguments(asp):
    out = (ctypes.c_int64 * 4)()
    assert asp._L.as_batch_sweep_counters(None, out, 4) == asp._lib.AS_EINVAL
    assert asp._L.as_search_batch_taus(None, None, None, 0, 0, None, 0, None, None, None, None, None) == asp._lib.AS_EINVAL
