"""Workload for the kernel statistics of the per-query list forms (profiles/r11_lists_kernel_stats.csv), run as
rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lists_kernel_stats.py
At 1M x 768 (tools/lists_bench.py's index, queries and lists): B = 1024 lists of C = 100 and of C = 1000 candidates through
`score_lists_batch` (lists_score_kernel), six calls each, and THE SAME ROWS as one flat id list through `score_items`
(subset_score_kernel: one query, the same row bytes), six calls each -- the two kernels' durations side by side per size."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import pyarrowspace_amd as asp  # noqa: E402
from lists_bench import draw_list  # noqa: E402
from tau_sweep_bench import gpu_clustered  # noqa: E402


def main():
    n, d, tau = 1_000_000, 768, 0.62
    X = gpu_clustered(n, d, 42)
    gp = {"eps": bench.calibrate_eps(X, 25), "k": 25, "topk": 15, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build_from_device(gp, X.data_ptr(), "float32", n, d, d)
    Q = np.ascontiguousarray(np.stack([np.ascontiguousarray(q) for q in bench.make_queries(X, 1024, 43)]))
    del X
    torch.cuda.synchronize()
    rng = np.random.default_rng(45)
    q0 = np.ascontiguousarray(Q[0])
    for c in (100, 1000):
        lists = np.stack([draw_list(rng, n, c) for _ in range(1024)])
        for _ in range(6):
            aspace.score_lists_batch(Q, gl, tau, lists)
        flat = lists.reshape(-1)
        for _ in range(6):
            aspace.score_items(q0, gl, tau, flat)


if __name__ == "__main__":
    main()
