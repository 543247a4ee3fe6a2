"""CPU: tools/nibble_sim.py -- the numpy check behind the nibble tiles -- runs at a small N and reports a
coefficient below the window it computes.

4 000 x 768 rows of the GPU tests' recipe (16 centres, noise 0.3: cosine 0.92 inside a cluster), 8 queries of either kind.  What
must hold whatever the seed: the largest actual error of a coarse cosine lies within the coefficient the scan would be priced
with (the derivation of host_query_digits, by numbers); the coefficient lies below the lower edge of the scorer's window, and
that edge above every cosine between a query and a row of another cluster -- so the 4-bit operand keeps exactly the rows the
8-bit one keeps."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "nibble_sim.py")


def test_tool_runs_and_reports_a_coefficient_below_its_window():
    p = subprocess.run([sys.executable, TOOL, "--n", "4000", "--nclust", "16", "--noise", "0.3", "--queries", "8"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print({k: v for k, v in out.items() if k != "queries"})
    assert len(out["queries"]) == 16
    assert 0.0 < out["r4_mean"] <= out["r4_max"] < 0.25
    assert out["r4_max"] <= out["coef4_max"] < out["window_low_min_bits4"]
    assert out["cross_cluster_cos_max"] < out["window_low_min_bits4"]
    assert out["err4_max"] <= out["coef4_max"] and out["err8_max"] <= out["coef8_max"]
    assert out["coefficient_below_window"] and out["window_clear_of_other_clusters"] and out["error_within_coefficient"]
    assert out["same_scorer_candidates"] and out["ok"]
    for r in out["queries"]:
        assert r["bits4"]["scorer_candidates"] == r["bits8"]["scorer_candidates"] > 0


def test_quantiser_levels_and_clip_choice():
    """quantise_rows, the reference of tests/test_gpu_nibble_image.py: levels in [-8, 7], the reconstruction within half a step
    of every element the clip does not cut, and the clip factor chosen is the one of least residual."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import nibble_sim
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((64, 96)).astype(np.float32)
    X[3] = 1.0                       # all-equal columns
    X[4, 7] = 1.0e4                  # one huge outlier
    lv, t, best, res = nibble_sim.quantise_rows(X)
    assert lv.min() >= -8 and lv.max() <= 7
    assert (res[np.arange(64), best] == res.min(axis=1)).all()
    xt = nibble_sim.dequantise(lv, t)
    inside = np.abs(X) < 7.5 * t[:, None]
    assert (np.abs(xt - X)[inside] <= 0.5 * t[:, None].repeat(96, 1)[inside] * (1 + 1e-6)).all()
    assert (lv[3] == lv[3, 0]).all() and lv[3, 0] == 7          # the maximum sits on the top level at every clip factor
    assert lv[4, 7] == 7                                        # the outlier sits on the top level, clipped or not
