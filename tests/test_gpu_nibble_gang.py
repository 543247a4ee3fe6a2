"""GPU: a search prepared for the nibble tiles is never filed into a gang scan (the gang kernel reads the 8-bit tiles, 8-bit query
digits and the FIRST member's row scales for every member).

query_begin decides for the tiles while no concurrent caller has been seen lately (gang_hint <= 0); a second thread that enters
as_search after that decision raises the hint, and the same search must then still scan alone (query_begin's `why`, gang_launch and
launch_scan_gang each hold it).  The test drives that lone-to-concurrent transition over and over under forced 4 on a small
index: 70 searches of one thread (the hint of the last burst runs out: the tiles are read again), then four threads started
together -- native threads against the C ABI (no interpreter lock between their calls: the driver checks every best hit), then
Python threads (every hit list and score compared with the serial answer, element for element).  Whatever the interleaving:
no call fails (launch_scan_gang refuses a nibble member with an error), every answer is the serial one bit for bit, the lone
phases did read the nibble tiles, and scans of two and more members did form."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nibble_searches_never_join_a_gang_across_lone_to_concurrent_transitions():
    import pyarrowspace_amd as asp
    from test_gpu_nibble_scan import make_data
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import thread_bench
    finally:
        sys.path.pop(0)
    asp.enable_search_stats(False)     # (process-global; a scan that is timed per launch is not shared)
    X, gp, qs, _ = make_data(4133, 544, "l2")
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(21)
    d = X.shape[1]
    Q = np.ascontiguousarray(X[rng.integers(0, len(X), 48)] + 0.02 * rng.standard_normal((48, d)) / np.sqrt(d))
    try:
        assert asp._L.as_set_tuning(b"coarse_bits", 8) == 0
        want = [aspace.search(q, gl, 0.62) for q in Q]
        assert aspace.last_scan_bits == 8
        first = np.array([w[0][0] for w in want], dtype=np.int64)
        assert asp._L.as_set_tuning(b"coarse_bits", 4) == 0
        bad, shared, lone_nibble = [], 0, 0

        def worker(t):
            try:
                for i in range(25):
                    j = (t * 13 + i) % len(Q)
                    if aspace.search(Q[j], gl, 0.62) != want[j]:
                        bad.append((t, i, j))
            except BaseException as e:   # noqa: BLE001
                bad.append(repr(e))

        for rnd in range(6):
            c0 = aspace.search_counters()
            for i in range(70):
                j = (rnd * 7 + i) % len(Q)
                assert aspace.search(Q[j], gl, 0.62) == want[j], (rnd, i)
            lone_nibble += aspace.search_counters()["nibble_scans"] - c0["nibble_scans"]
            if rnd % 2 == 0:
                rate, errs, gangs = thread_bench.native_rate(aspace, gl, Q, 0.62, 4, 40, first)
                assert errs == 0 and rate > 0, (rnd, errs)
                shared += sum(gangs[1:])
            else:
                g0 = aspace.gang_counters()
                ths = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()
                shared += sum(b - a for a, b in zip(g0[1:], aspace.gang_counters()[1:]))
            assert not bad, bad[:5]
        c = aspace.search_counters()
        print(f"nibble scans in the lone phases {lone_nibble}, scans with 2+ members {shared}, counters {c}, skips {aspace.gang_skips()}")
        assert lone_nibble > 0 and shared > 0
    finally:
        assert asp._L.as_set_tuning(b"coarse_bits", -1) == 0
