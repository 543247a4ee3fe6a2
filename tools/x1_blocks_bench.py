"""Blocks of the fused tail's first kernel (as_set_tuning("x1_blocks", v)) at the headline shape, one index, one process:
rounds of timed single searches under 64 / 128 / 256 blocks, interleaved, for both positions of "x1_final_rank".
    python tools/x1_blocks_bench.py [--n 1000000 --d 768 --k 25 --topk 15 --rounds 3 --steps 300]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--topk", type=int, default=15)
    ap.add_argument("--tau", type=float, default=0.62)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    import pyarrowspace_amd as asp
    X = bench.make_data(a.n, a.d, 42, "cuda")
    gp = {"eps": bench.calibrate_eps(X, a.k), "k": a.k, "topk": a.topk, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", a.n, a.d, a.d)
    Q = [np.ascontiguousarray(q) for q in bench.make_queries(X, a.steps + 30, 43)]
    first = None
    try:
        for rnd in range(a.rounds):
            for fr in (0, 1):
                for blocks in (64, 128, 256):
                    assert asp._L.as_set_tuning(b"x1_final_rank", fr) == 0 and asp._L.as_set_tuning(b"x1_blocks", blocks) == 0
                    for q in Q[:30]:
                        aspace.search(q, gl, a.tau)
                    t0 = time.perf_counter()
                    for q in Q[30:]:
                        aspace.search(q, gl, a.tau)
                    dt = time.perf_counter() - t0
                    got = [aspace.search(q, gl, a.tau) for q in Q[:8]]
                    first = first or got
                    assert got == first      # (results never depend on either setting)
                    print(f"round {rnd} x1_final_rank={fr} x1_blocks={blocks}: {a.steps / dt:.1f} queries/s, {1e3 * dt / a.steps:.5f} ms per search, operand {aspace.last_scan_operand}", flush=True)
    finally:
        asp._L.as_set_tuning(b"x1_final_rank", -1)
        asp._L.as_set_tuning(b"x1_blocks", 128)
    print("reruns", aspace.search_counters())


if __name__ == "__main__":
    main()
