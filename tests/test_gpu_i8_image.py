"""GPU: the int8 two-digit image as it lies in device memory (space_i8_image / space_i8h_image through ArrowSpace.debug_i8_image)
and the two maxima the quantiser measures, against the numpy quantiser (tools/i8_sim.py: the kernel's fp32 arithmetic operation
by operation) and fp64.  The rows: tests/i8_image_ref.py (checked on the CPU by tests/test_i8_image_inputs.py).

  a. digits and scales: a1 in bytes 0-63 and a2 in bytes 64-127 of every 128-byte slab row equal the numpy quantiser's, columns from
     d to dp8 hold digit 0, padding rows are zero with scale 0, and fa8 is the reference's bit for bit.
  b. the high-digit tiles: the byte at [row // 64][c // 16][row % 64][c % 16] is a1 of (row, c), padding included.
  c. U and V: what debug_i8_image reports is what as_ring_i8_stats reports on a space made the way the ring makes one, and both are
     upper bounds of the true values, and tight ones.  With U_true = max_i s_i |theta_i|_2 / (16256 |x_i|), theta = 16256 x / s - q
     over all dp8 columns, and V_true = max_i s_i |a2_i|_2 / (16256 |x_i|), both in fp64 from the digits read back over the rows of
     nonzero norm, and u = 2^-24:

         U_true (1.001 - dp8 u) <= U_gpu <= (U_true + 0.004 sqrt(dp8) max_i s_i / (16256 |x_i|)) 1.001 (1 + c dp8 u)
         V_true (1.001 - dp8 u) <= V_gpu <= V_true 1.001 (1 + c dp8 u),            c = 1.

     Where they come from.  The kernel forms per row  fl(fl(fl(m fl(sqrt(S))) / fl(16256 fl(sqrt(n32)))) 1.001f)  with S an fp32 sum
     of dp8 terms: th^2, th = fl(|sc - q| + 0.004f) (sc - q is exact), or a2^2 (exact).  Upper limit: |th|_2 <= |theta|_2 +
     0.004 sqrt(dp8) by the triangle inequality, then the kernel's x 1.001, then the roundings: a term th^2 carries at most 5 u (0.004f,
     the sum that makes th -- both twice in the square -- and the product), a sum of dp8 non-negative terms in ANY order at most
     (dp8 - 1) u more, the square root halves that and adds u, m * sqrt one u, sqrt(n32) 1.5 u (n32 is a rounded fp64 norm), the
     product with 16256, the division, 1.001f and the last product one u each: (dp8 / 2 + 9.5) u to first order, below dp8 u with the
     second-order terms for every dp8 >= 64 -- hence c = 1, derived, not measured.  Lower limit: the x 1.001 is the margin that keeps
     the fp32 result above the true value whatever the roundings (th >= |theta| column by column: the +0.004 exceeds the 0.002 by
     which fl(x * inv) can be off), so at least 1.001 less the same dp8 u of it must be there.  An over-inflated maximum (a word
     that was never initialised) fails the upper limits, a lost row (a later trip of the grid-stride loop that does not count, or one
     that overwrites an earlier one: the 8300-row sets) or a missing margin the lower ones.
  d. the bound itself: with t = 128 a1.b1 + a1.b2 + a2.b1 in exact integers and fa8 widened to fp64,
     |t fa_i fa_j - x_i.x_j| <= coef |x_i||x_j| for every pair of rows of nonzero norm, coef = oracle_np.ring_coef_i8(U_gpu, V_gpu), x the
     fp32-rounded items in fp64; pairs with the zero row have error exactly 0.
  e. the gate: whole indexes built from the row sets (without the zero row) run their k-NN block on the int8 pipe where the
     coefficient lies under 1e-3 and on the bf16 pipe where it lies over, and are the fp64 oracle's either way; so are plain
     clustered rows scaled to the inner edges of the fp32-safe band (1e-15, 1e18), on the int8 pipe.
  f. the dots the two 8-bit single-query scans keep (the high digits alone, and the two-digit image) differ from the fp64 dots by
     at most the coefficient they are priced with, on every row."""
import functools
import os

import numpy as np
import pytest

import i8_image_ref as ref
from conftest import calibrate_eps, clustered
from oracle import oracle_np

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
C_ROUND = 1.0          # (derived above)


@functools.lru_cache(maxsize=None)
def built(name):
    """the row set as an index (zero row and all), its image read back -- made once, shared, not to be changed"""
    import pyarrowspace_amd as asp
    X, special = ref.make_set(name)
    gp = {"eps": 0.4, "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    img = aspace.debug_i8_image()
    assert img is not None and img["bad"] == 0
    for v in img.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return aspace, gl, img


@pytest.mark.parametrize("name", ref.SETS)
def test_digits_and_scales_match_the_numpy_quantiser(name):
    X, special = ref.make_set(name)
    r = ref.reference(name)
    n, d = X.shape
    _, _, img = built(name)
    dp8, rows = img["dp8"], img["rows"]
    assert dp8 == (d + 63) // 64 * 64 == r["a1"].shape[1]
    assert rows == (n + ref.ROW_TILE - 1) // ref.ROW_TILE * ref.ROW_TILE + ref.ROW_TILE
    assert img["x8"].shape == (rows, dp8 // 64, 2, 64) and img["fa8"].shape == (rows,)
    a1, a2 = ref.digits_of_image(img["x8"])
    assert not a1[n:].any() and not a2[n:].any() and not img["fa8"][n:].any()         # padding rows
    assert not a1[:, d:].any() and not a2[:, d:].any()                                 # padded columns
    bad = np.flatnonzero((a1[:n] != r["a1"]).any(axis=1) | (a2[:n] != r["a2"]).any(axis=1))
    assert len(bad) == 0, (bad[:8], {k: v for k, v in special.items() if v in set(bad.tolist())})
    fa = np.ascontiguousarray(img["fa8"][:n])
    diff = np.flatnonzero(fa.view(np.uint32) != r["fa8"].view(np.uint32))
    assert len(diff) == 0, (diff[:8], fa[diff[:8]], r["fa8"][diff[:8]])
    if "zero" in special:
        assert fa[special["zero"]] == 0.0 and not a1[special["zero"]].any() and not a2[special["zero"]].any()


@pytest.mark.parametrize("name", ref.SETS)
def test_high_digit_tiles_hold_a1_of_every_row_and_column(name):
    _, _, img = built(name)
    a1, _ = ref.digits_of_image(img["x8"])
    rows, dp8 = a1.shape
    assert img["x8h"].shape == (rows // 64, dp8 // 16, 64, 16)
    want = ref.tiles_of_digits(a1)
    assert np.array_equal(img["x8h"], want), np.argwhere(img["x8h"] != want)[:8]
    # (the layout, spelled out on a few bytes: rows of the first, a middle and the last tile, the first and the last chunk)
    for row in (0, 63, 64, rows // 2 + 5, rows - 1):
        for c in (0, 15, 16, dp8 - 17, dp8 - 1):
            assert img["x8h"][row // 64, c // 16, row % 64, c % 16] == a1[row, c]


def _ring_stats(X):
    """U, V, unusable as a rank of the ring measures them: a space made the way pyarrowspace_amd/dist.py makes one"""
    import torch
    from pyarrowspace_amd.dist import HipEngine
    e = HipEngine({"eps": 0.4, "k": 8, "topk": 5, "p": 2.0, "sigma": None})
    try:
        e.create_space(torch.from_numpy(np.ascontiguousarray(X.astype(np.float32))).cuda())
        return e.ring_i8_stats()
    finally:
        e.close()


@pytest.mark.parametrize("name", ref.SETS)
def test_maxima_are_upper_bounds_and_tight(name):
    X, special = ref.make_set(name)
    n, d = X.shape
    _, _, img = built(name)
    dp8 = img["dp8"]
    su, sv, unusable = _ring_stats(X)
    assert (su, sv, unusable) == (img["u"], img["v"], 0.0)
    assert img["coef"] == oracle_np.ring_coef_i8(img["u"], img["v"])
    a1, a2 = ref.digits_of_image(img["x8"])
    u_true, v_true, ratio = ref.sim().true_maxima(X.astype(np.float32), a1[:n], a2[:n], dp8)
    U, V = float(u_true.max()), float(v_true.max())
    rnd = C_ROUND * dp8 * U24
    u_hi = (U + 0.004 * np.sqrt(dp8) * float(ratio.max())) * 1.001 * (1.0 + rnd)
    v_hi = V * 1.001 * (1.0 + rnd)
    print(f"{name} (dp8 {dp8}): U_gpu {img['u']:.6e} = {img['u'] / U:.6f} U_true = {img['u'] / u_hi:.6f} of its upper limit (row {int(u_true.argmax())}); "
          f"V_gpu {img['v']:.6e} = {img['v'] / V:.8f} V_true = {img['v'] / v_hi:.8f} of its upper limit (row {int(v_true.argmax())})")
    assert U * (1.001 - rnd) <= img["u"] <= u_hi
    assert V * (1.001 - rnd) <= img["v"] <= v_hi


@pytest.mark.parametrize("name", ref.SETS)
def test_every_pair_of_rows_lies_within_the_coefficient(name):
    X, special = ref.make_set(name)
    n = X.shape[0]
    _, _, img = built(name)
    a1, a2 = ref.digits_of_image(img["x8"])
    coef = oracle_np.ring_coef_i8(img["u"], img["v"])
    worst, at, dead = ref.sim().pair_errors(X.astype(np.float32), a1[:n], a2[:n], img["fa8"][:n])
    print(f"{name}: largest |t fa_i fa_j - x_i.x_j| / (|x_i||x_j|) {worst:.4e} = {worst / coef:.4f} of the coefficient {coef:.4e}, at rows {at}")
    assert worst <= coef
    assert dead == 0.0                       # pairs with the zero row


def _check_gate(X, gp, oracle_lib, int8):
    import pyarrowspace_amd as asp
    from test_gpu_parity import _check_index
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    img = aspace.debug_i8_image()
    assert img is not None
    print(f"coefficient {img['coef']:.4e}, pipe {aspace.knn_pipe}")
    if int8:
        assert aspace.knn_pipe == "int8" and img["coef"] <= 1.0e-3
    else:
        assert aspace.knn_pipe == "bf16" and img["coef"] > 1.0e-3
    _check_index(aspace, gl, oracle_lib.OracleIndex(X, gp))       # lambdas, degrees, CSR: test_gpu_parity's comparison (its RTOL, atol 1e-300)


@pytest.mark.parametrize("name", ref.SETS)
def test_the_gate_picks_the_pipe_and_the_index_is_the_oracles(oracle_lib, name):
    X, special = ref.make_set(name)
    if "zero" in special:
        X = np.ascontiguousarray(np.delete(X, special["zero"], axis=0))
    gp = {"eps": calibrate_eps(X, 6), "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    _check_gate(X, gp, oracle_lib, ref.GATE_INT8[name])


@pytest.mark.parametrize("scale", [1e-15, 1e18])
def test_rows_at_the_inner_edges_of_the_safe_band_stay_on_int8(oracle_lib, scale):
    """squared norms of 1e-30 and 1e36, just inside [2^-100, 2^120]: the products of two scales fa_i fa_j come near the fp32 denormals
    at the low edge"""
    X = clustered(700, 96, nclust=8, noise=0.3, seed=5)
    gp = {"eps": calibrate_eps(X, 6) * scale, "k": 6, "topk": 5, "p": 2.0, "sigma": None}
    n64 = ((X * scale) ** 2).sum(axis=1)
    assert 2.0 ** -100 < n64.min() < 2.0 ** -99 or 2.0 ** 119 < n64.max() < 2.0 ** 120
    _check_gate(X * scale, gp, oracle_lib, True)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_kept_dots_of_both_8_bit_scans_lie_within_their_coefficients():
    import pyarrowspace_amd as asp
    from test_gpu_nibble_scan import make_data
    X, gp, qs, _ = make_data(4133, 544, "l2")
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(3)
    d = X.shape[1]
    own = (X @ X[0]) > 0.8
    centre = _unit(X[own].mean(axis=0))
    queries = [_unit(X[i] + 0.02 * rng.standard_normal(d) / np.sqrt(d)) for i in (1, 500, 2000, 4132)]
    queries += [_unit(centre * np.sqrt(d) + 0.3 * rng.standard_normal(d)) * s for s in (1.0, 3.0, 0.25, 1.0)]
    X64 = X.astype(np.float32).astype(np.float64)
    nx = np.linalg.norm(X64, axis=1)
    saved = os.environ.get("ARROWSPACE_SCAN_COARSE")
    coefs = {}
    try:
        assert asp._L.as_set_tuning(b"coarse_bits", 8) == 0
        for operand, env in (("int8-high", None), ("int8", "0")):
            if env is None:
                os.environ.pop("ARROWSPACE_SCAN_COARSE", None)
            else:
                os.environ["ARROWSPACE_SCAN_COARSE"] = env          # (read per call)
            for j, q in enumerate(queries):
                q = np.ascontiguousarray(q)
                try:
                    aspace.search(q, gl, 0.62)
                except asp.PanicException:      # (a scaled query is far from every row in L2: the scan ran all the same)
                    assert abs(np.linalg.norm(q) - 1.0) > 0.1
                assert aspace.last_scan_operand == operand and aspace.last_scan_bits == 8, (operand, j)
                dots, coef = aspace.debug_last_dots()
                err = np.abs(dots.astype(np.float64) - X64 @ q) / (nx * np.linalg.norm(q))
                print(f"{operand}, query {j}: coefficient {coef:.4e}, largest |dot - x.q| / (|x||q|) {err.max():.4e} = {err.max() / coef:.4f} of it")
                assert (err <= coef).all(), (operand, j, int(err.argmax()))
                coefs[operand, j] = coef
        for j in range(len(queries)):
            assert coefs["int8", j] < coefs["int8-high", j] <= 4.0e-2
    finally:
        assert asp._L.as_set_tuning(b"coarse_bits", -1) == 0
        if saved is None:
            os.environ.pop("ARROWSPACE_SCAN_COARSE", None)
        else:
            os.environ["ARROWSPACE_SCAN_COARSE"] = saved
