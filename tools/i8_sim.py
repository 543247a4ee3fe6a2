#!/usr/bin/env python3
"""Numpy reference of the int8 two-digit image (as_k2bf.hip, quant_i8_kernel), no GPU.

quantise_rows(X32, dp8) follows the kernel's fp32 arithmetic operation by operation -- m = max|x|, inv = 16256 / m (0 for a zero
row), sc = x * inv, q = clamp(rint(sc), +-16256) (round half to even), a2 = ((q + 64) mod 128) - 64, a1 = (q - a2) / 128, the
scale fa8 = m * (sqrt(128) / 16256) -- so the digits and the scales are expected bit for bit.  It also forms the kernel's own fp32
estimates of the two maxima (the residues with +0.004 on every one of the dp8 columns, a lane's columns summed in turn and the 64
lanes by a butterfly, x 1.001; the device may fuse a product into the sum that follows it, so these agree to rounding, not to
the bit), and, separately, the TRUE per-row values in fp64 from the digits:

    theta = 16256 x / s - q over all dp8 columns,  U_i = s_i |theta_i|_2 / (16256 |x_i|),  V_i = s_i |a2_i|_2 / (16256 |x_i|).

pair_errors(...) gives the largest |t fa_i fa_j - x_i.x_j| / (|x_i||x_j|), t = 128 a1.b1 + a1.b2 + a2.b1 in exact integers, over
all pairs of rows: what 2.001 U + V^2 + 12 * 2^-24 has to cover.

    python tools/i8_sim.py --n 4000 --d 768        # clustered unit rows: U, V, the coefficient and the largest actual error
"""
import argparse
import json
import sys

import numpy as np

QMAX = 16256          # 127 * 128
FA_CONST = np.float32(11.313708498984761) / np.float32(16256.0)      # the kernel's constant: sqrt(128) / 16256 in fp32


def true_maxima(X32, a1, a2, dp8=None):
    """fp64, from the digits: (U_i, V_i, s_i / (16256 |x_i|)) per row (0 where the row's norm is 0); theta over all columns of the
    digits given (the padded ones hold x = 0, q = 0)."""
    X64 = np.asarray(X32, dtype=np.float32).astype(np.float64)
    n, d = X64.shape
    cols = a1.shape[1]
    q = 128.0 * a1.astype(np.float64) + a2.astype(np.float64)
    s = np.abs(X64).max(axis=1)
    nx = np.sqrt((X64 * X64).sum(axis=1))
    ok = nx > 0.0
    ss = np.where(ok, s, 1.0)
    theta = -q
    theta[:, :d] += float(QMAX) * X64 / ss[:, None]
    r = np.where(ok, s / (float(QMAX) * np.where(ok, nx, 1.0)), 0.0)
    U = r * np.sqrt((theta * theta).sum(axis=1))
    V = r * np.sqrt((a2.astype(np.float64) ** 2).sum(axis=1))
    assert cols >= d and (dp8 is None or cols == dp8)
    return np.where(ok, U, 0.0), np.where(ok, V, 0.0), r


def _wave_sum(t):
    """fp32 sum of [n, dp8] as the kernel's wave forms it: lane l adds its columns l, l + 64, ... in turn, then a butterfly"""
    n, dp8 = t.shape
    t = t.reshape(n, dp8 // 64, 64)
    acc = np.zeros((n, 64), dtype=np.float32)
    for j in range(dp8 // 64):
        acc = acc + t[:, j, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def quantise_rows(X32, dp8=None):
    """-> dict: a1, a2 (int8 [n, dp8]), q (int32), fa8, m (float32 [n]), u_est, v_est (float32 [n]: the kernel's own per-row
    estimates, 0 for a row of norm 0), U_est, V_est (their maxima), u_true, v_true, ratio (float64 [n]), U_true, V_true."""
    X32 = np.ascontiguousarray(X32, dtype=np.float32)
    n, d = X32.shape
    if dp8 is None:
        dp8 = (d + 63) // 64 * 64
    assert dp8 % 64 == 0 and dp8 >= d
    m = np.abs(X32).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(m > 0, np.float32(QMAX) / m, np.float32(0.0)).astype(np.float32)
    xp = np.zeros((n, dp8), dtype=np.float32)
    xp[:, :d] = X32
    with np.errstate(over="ignore", invalid="ignore"):
        sc = (xp * inv[:, None]).astype(np.float32)
    q = np.clip(np.rint(sc), -QMAX, QMAX).astype(np.int32)
    a2 = ((q + 64 + (1 << 20)) & 127) - 64
    a1 = (q - a2) >> 7
    assert np.abs(a1).max(initial=0) <= 127 and a2.min(initial=0) >= -64 and a2.max(initial=0) <= 63
    fa8 = (m * FA_CONST).astype(np.float32)
    # the kernel's estimates
    th = (np.abs(sc - q.astype(np.float32)).astype(np.float32) + np.float32(0.004)).astype(np.float32)
    st2 = _wave_sum((th * th).astype(np.float32))
    sa2 = _wave_sum((a2 * a2).astype(np.float32))
    n64 = (X32.astype(np.float64) ** 2).sum(axis=1)
    nx = np.sqrt(n64.astype(np.float32)).astype(np.float32)
    live = nx > 0
    den = np.where(live, np.float32(QMAX) * nx, np.float32(1.0)).astype(np.float32)
    u_est = np.where(live, ((m * np.sqrt(st2)).astype(np.float32) / den).astype(np.float32) * np.float32(1.001), np.float32(0.0)).astype(np.float32)
    v_est = np.where(live, ((m * np.sqrt(sa2)).astype(np.float32) / den).astype(np.float32) * np.float32(1.001), np.float32(0.0)).astype(np.float32)
    u_true, v_true, ratio = true_maxima(X32, a1, a2, dp8)
    return {"a1": a1.astype(np.int8), "a2": a2.astype(np.int8), "q": q, "fa8": fa8, "m": m, "u_est": u_est, "v_est": v_est,
            "U_est": float(u_est.max(initial=0.0)), "V_est": float(v_est.max(initial=0.0)), "u_true": u_true, "v_true": v_true,
            "ratio": ratio, "U_true": float(u_true.max(initial=0.0)), "V_true": float(v_true.max(initial=0.0))}


def coef_i8(U, V):
    """err_coef_i8 (as_build.hip): what a product of two rows of the image is priced with, relative to |x_i||x_j|"""
    return 2.001 * U + V * V + 12.0 * 2.0 ** -24


def pair_errors(X32, a1, a2, fa8, block=1024):
    """-> (largest |t fa_i fa_j - x_i.x_j| / (|x_i||x_j|) over the pairs of rows with nonzero norms and its (i, j), largest
    |t fa_i fa_j - x_i.x_j| over the pairs with a row of norm 0).  t in exact integers (fp64 holds them: |t| < 2^53), fa8 widened."""
    X64 = np.asarray(X32, dtype=np.float32).astype(np.float64)
    n, d = X64.shape
    A1, A2 = a1.astype(np.float64), a2.astype(np.float64)
    fa = fa8.astype(np.float64)
    nx = np.sqrt((X64 * X64).sum(axis=1))
    live = nx > 0
    worst, at, dead = 0.0, (0, 0), 0.0
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        t = 128.0 * (A1[r0:r1] @ A1.T) + A1[r0:r1] @ A2.T + A2[r0:r1] @ A1.T
        err = np.abs(t * fa[r0:r1, None] * fa[None, :] - X64[r0:r1] @ X64.T)
        both = live[r0:r1, None] & live[None, :]
        if (~both).any():
            dead = max(dead, float(err[~both].max()))
        rel = np.where(both, err / np.where(both, nx[r0:r1, None] * nx[None, :], 1.0), 0.0)
        k = int(rel.argmax())
        if rel.flat[k] > worst:
            worst, at = float(rel.flat[k]), (r0 + k // n, k % n)
    return worst, at, dead


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nclust", type=int, default=16)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    C = rng.standard_normal((a.nclust, a.d))
    X = C[rng.integers(0, a.nclust, a.n)] + a.noise * rng.standard_normal((a.n, a.d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X32 = X.astype(np.float32)
    r = quantise_rows(X32)
    worst, at, _ = pair_errors(X32, r["a1"], r["a2"], r["fa8"])
    coef = coef_i8(r["U_est"], r["V_est"])
    out = {"n": a.n, "d": a.d, "dp8": int(r["a1"].shape[1]), "U_est": r["U_est"], "V_est": r["V_est"], "U_true": r["U_true"],
           "V_true": r["V_true"], "coef": coef, "usable": bool(coef <= 1.0e-3), "max_pair_error": worst, "at": list(at),
           "ok": bool(worst <= coef and r["U_true"] <= r["U_est"] and r["V_true"] <= r["V_est"])}
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
