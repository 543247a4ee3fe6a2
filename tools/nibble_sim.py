#!/usr/bin/env python3
"""CPU check of the nibble tiles, numpy only, no GPU: would a 4-bit coarse operand keep the single query's
candidate sets as small as the 8-bit one does?

On the bench recipe (bench.py, make_data: default_rng(seed), `nclust` centres, noise 0.5, rows normalised, fp32) at N rows it
quantises the items as space_nib_image does (quantise_rows below: the same arithmetic in fp32, operation by operation),
quantises the queries to their high digit q1 as host_query_digits does, and reports

  * the items' coefficient R4 = max_i |x_i - x~_i| / |x_i| (and the mean), the query part u_q + v_q, and the coefficient the
    scan is priced with, R4 + (1 + R4)(u_q + v_q);
  * the largest actual error of a coarse cosine over all (query, row) pairs;
  * per query the scorer's candidates -- rows with a coarse cosine at or above (bound - W - 2 coef), W = (1 - tau) / (2 tau),
    bound = the lower edge of the cosine bin (width 1/32) of the M-th largest coarse cosine, M = topk rounded up to 64 as the
    workspace does -- and the k-NN prefilter's -- rows inside the eps ball widened by coef -- for 8 bits (the high digit a1 of
    the two-digit image against q1, q2) and for 4 bits;
  * the window's lower edge against the largest cosine between a query and a row of another cluster than its own.

Two query kinds as in bench.py: perturbed items and fresh draws around the centres (default_rng(seed + 1)).
Prints one JSON line; exit status 1 unless the 4-bit coefficient lies below the window's lower edge, that edge lies above every
cross-cluster cosine, and no actual error exceeds its coefficient ("ok").

    python tools/nibble_sim.py --n 200000            # the figures of DESIGN.md 5.4 (a minute of numpy)
    python tools/nibble_sim.py --n 4000 --nclust 16 --noise 0.3  # what tests/test_nibble_sim.py runs (the GPU tests' recipe)
"""
import argparse
import json
import sys

import numpy as np

CLIPS = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5)


def quantise_rows(X32, d=None):
    """The quantiser of space_nib_image in numpy fp32: per row t = f max|x| / 7.5 with the clip factor f of CLIPS that leaves
    the smallest residual (the first of equals), lv = clamp(floor(x / t), -8, 7) with value (lv + 1/2) t.
    Returns (lv int8 [n, d], t float32 [n], f index [n], residual^2 float32 [n, 6])."""
    X32 = np.ascontiguousarray(X32, dtype=np.float32)
    if d is None:
        d = X32.shape[1]
    m = np.abs(X32).max(axis=1)
    n = X32.shape[0]
    res = np.empty((n, len(CLIPS)), dtype=np.float32)
    ts = np.empty((n, len(CLIPS)), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j, f in enumerate(CLIPS):
            t = (np.float32(f) * m) / np.float32(7.5)
            lv = np.clip(np.floor(X32 / t[:, None]), -8, 7).astype(np.float32)
            r = X32 - (lv + np.float32(0.5)) * t[:, None]
            res[:, j] = (r * r).sum(axis=1, dtype=np.float32)
            ts[:, j] = t
        best = np.argmin(res, axis=1)            # (the first of equals, as the kernel's strict `<`)
        t = ts[np.arange(n), best]
        lv = np.clip(np.floor(X32 / t[:, None]), -8, 7).astype(np.int8)
    return lv, t, best, res


def dequantise(lv, t):
    return (lv.astype(np.float64) + 0.5) * t.astype(np.float64)[:, None]


def query_digits(q):
    """host_query_digits: q ~ s (128 q1 + q2) / 16256, s = max|q|; returns (q1, q2, s, u_q, v_q)"""
    q32 = q.astype(np.float32)
    s = float(np.abs(q32).max())
    sc = q32.astype(np.float64) * (16256.0 / s)
    qq = np.clip(np.rint(sc), -16256, 16256).astype(np.int64)
    q2 = ((qq + 64 + (1 << 20)) & 127) - 64
    q1 = (qq - q2) >> 7
    nq = float(np.linalg.norm(q))
    uq = s * float(np.linalg.norm(np.abs(sc - qq) + 0.004)) / (16256.0 * nq)
    vq = s * float(np.linalg.norm(q2)) / (16256.0 * nq)
    return q1, q2, s, uq, vq


def items_8bit(X32):
    """the two-digit image's high digit: x ~ s 128 a1 / 16256; returns (a1 as float64 values, V = max |a2 part| / |x|, U)"""
    s = np.abs(X32).max(axis=1).astype(np.float64)
    sc = X32.astype(np.float64) * (16256.0 / s)[:, None]
    q = np.clip(np.rint(sc), -16256, 16256)
    a2 = ((q.astype(np.int64) + 64 + (1 << 20)) & 127) - 64
    a1 = (q - a2) / 128.0
    nx = np.linalg.norm(X32.astype(np.float64), axis=1)
    V = float((s * np.linalg.norm(a2, axis=1) / (16256.0 * nx)).max())
    U = float((s * np.linalg.norm(np.abs(sc - q) + 0.004, axis=1) / (16256.0 * nx)).max())
    return a1 * (128.0 * s / 16256.0)[:, None], U, V


def bin_edge(c):
    return np.floor((c + 1.0) * 32.0) / 32.0 - 1.0


def simulate(n, d, nclust, nq, tau, k, topk, seed, eps=None, noise=0.5):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((nclust, d))
    z = rng.integers(0, nclust, n)
    X = C[z] + noise * rng.standard_normal((n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X32 = X.astype(np.float32)
    X64 = X32.astype(np.float64)
    nx = np.linalg.norm(X64, axis=1)
    rq = np.random.default_rng(seed + 1)
    rows = rq.integers(0, n, nq)
    Qp = X64[rows] + 0.02 * rq.standard_normal((nq, d)) / np.sqrt(d)
    zq = rq.integers(0, nclust, nq)
    Qd = C[zq] + noise * rq.standard_normal((nq, d))
    Q = np.concatenate([Qp, Qd])
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    kinds = ["perturbed"] * nq + ["in_distribution"] * nq
    if eps is None:   # mean degree 2 k before the cap (bench.py, calibrate_eps), from a row sample
        sample = rng.choice(n, size=min(256, n), replace=False)
        D = np.sqrt(np.maximum(2.0 - 2.0 * (X64[sample] @ X64.T), 0.0))
        D[np.arange(len(sample)), sample] = np.inf
        eps = float(np.quantile(D[np.isfinite(D)], min(1.0, 2.0 * k / max(n - 1, 1))))
    lv, t, best, _ = quantise_rows(X32)
    X4 = dequantise(lv, t)
    r4 = np.linalg.norm(X64 - X4, axis=1) / nx
    X8, U8, V8 = items_8bit(X32)
    M = (topk + 63) // 64 * 64
    W = (1.0 - tau) / (2.0 * tau)
    qclust = np.concatenate([z[rows], zq])
    cross = -1.0   # the largest cosine between a query and a row of another cluster than its own
    out = {"n": n, "d": d, "nclust": nclust, "tau": tau, "eps": eps, "r4_max": float(r4.max()), "r4_mean": float(r4.mean()),
           "clip_histogram": np.bincount(best, minlength=len(CLIPS)).tolist(), "queries": []}
    coef4_max = coef8_max = err4_max = err8_max = 0.0
    for qi in range(Q.shape[0]):
        q = Q[qi]
        q1, q2, s, uq, vq = query_digits(q)
        exact = (X64 @ q) / nx
        other = z != qclust[qi]
        if other.any():
            cross = max(cross, float(exact[other].max()))
        c4 = (X4 @ (q1 * (128.0 * s / 16256.0))) / nx
        c8 = (X8 @ ((128.0 * q1 + q2) * (s / 16256.0))) / nx
        coef4 = r4.max() * 1.001 + (1.0 + r4.max()) * (uq + vq) * 1.001
        coef8 = uq + 1.001 * U8 + 1.002 * V8
        rec = {"kind": kinds[qi]}
        for name, c, coef in (("bits8", c8, coef8), ("bits4", c4, coef4)):
            bound = bin_edge(np.sort(c)[-M]) if n >= M else -1.0
            sc_w = W + 2.0 * coef
            # k-NN prefilter, L2 on unit rows: |x - q|^2 = 2 - 2 cos <= eps^2 + coef (|x|^2 + |q|^2)
            knn = int(((2.0 - 2.0 * c) <= eps * eps + 2.0 * coef).sum())
            rec[name] = {"scorer_candidates": int((c >= bound - sc_w).sum()), "knn_candidates": knn, "window_low": float(bound - sc_w),
                         "coef": float(coef), "max_err": float(np.abs(c - exact).max())}
        out["queries"].append(rec)
        coef4_max, coef8_max = max(coef4_max, coef4), max(coef8_max, coef8)
        err4_max, err8_max = max(err4_max, rec["bits4"]["max_err"]), max(err8_max, rec["bits8"]["max_err"])
    out.update(coef4_max=float(coef4_max), coef8_max=float(coef8_max), err4_max=float(err4_max), err8_max=float(err8_max))
    for kind in ("perturbed", "in_distribution"):
        for bits in ("bits8", "bits4"):
            v = [r[bits]["scorer_candidates"] for r in out["queries"] if r["kind"] == kind]
            kn = [r[bits]["knn_candidates"] for r in out["queries"] if r["kind"] == kind]
            out[f"{kind}_{bits}"] = {"scorer_median": float(np.median(v)), "scorer_max": int(max(v)), "knn_median": float(np.median(kn)),
                                    "knn_max": int(max(kn))}
    out["window_low_min_bits4"] = float(min(r["bits4"]["window_low"] for r in out["queries"]))
    out["cross_cluster_cos_max"] = cross
    out["coefficient_below_window"] = bool(coef4_max < out["window_low_min_bits4"])
    out["window_clear_of_other_clusters"] = bool(out["window_low_min_bits4"] > cross)
    out["error_within_coefficient"] = bool(err4_max <= coef4_max and err8_max <= coef8_max)
    out["same_scorer_candidates"] = all(r["bits4"]["scorer_candidates"] == r["bits8"]["scorer_candidates"] for r in out["queries"])
    out["ok"] = bool(out["coefficient_below_window"] and out["window_clear_of_other_clusters"] and out["error_within_coefficient"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nclust", type=int, default=1024)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--queries", type=int, default=16, help="per query kind")
    ap.add_argument("--tau", type=float, default=0.62)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--topk", type=int, default=15)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--brief", action="store_true", help="leave the per-query records out of the JSON line")
    a = ap.parse_args(argv)
    out = simulate(a.n, a.d, a.nclust, a.queries, a.tau, a.k, a.topk, a.seed, noise=a.noise)
    if a.brief:
        out.pop("queries")
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
