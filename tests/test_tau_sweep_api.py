"""CPU: the tau-sweep extension's surface -- ArrowSpace.search_taus / sweep_counters (also under the reference module
name) and the C ABI symbols behind them.  No compute call: the GPU behaviour is tests/test_gpu_tau_sweep.py's."""
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


def test_arrowspace_has_search_taus_and_sweep_counters(asp):
    import arrowspace
    for cls in (asp.ArrowSpace, arrowspace.ArrowSpace):
        assert callable(getattr(cls, "search_taus", None))
        assert callable(getattr(cls, "sweep_counters", None))
    assert list(inspect.signature(asp.ArrowSpace.search_taus).parameters) == ["self", "item", "gl", "taus"]
    assert "Extension" in asp.ArrowSpace.search_taus.__doc__


def test_library_exports_the_sweep_symbols(asp):
    lib = ctypes.CDLL(asp._lib.LIB_PATH)
    for name in ("as_search_taus", "as_sweep_counters"):
        assert hasattr(lib, name)
        assert name in asp._lib.SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "arrowspace_hip.h")).read()
    assert "as_status as_search_taus(" in hdr and "as_status as_sweep_counters(" in hdr


def test_sweep_counters_reject_a_null_space(asp):
    out = (ctypes.c_int64 * 3)()
    assert asp._L.as_sweep_counters(None, out, 3) == asp._lib.AS_EINVAL
    assert asp._L.as_search_taus(None, None, None, 0, None, 0, None, None, None, None) == asp._lib.AS_EINVAL
