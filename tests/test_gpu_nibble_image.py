"""GPU: the nibble tiles as they lie in device memory (space_nib_image through ArrowSpace.debug_nibble_image) against the numpy
quantiser (tools/nibble_sim.py, quantise_rows: the kernel's fp32 arithmetic operation by operation).

  * tiles: every nibble equals the numpy quantiser's under the clip factor the kernel chose for the row.  That factor must be
    one of the six and its residual the smallest of the six in fp64 up to the rounding of an fp32 sum of d squares, (d - 1) 2^-23
    relative at most (1e-4 at d = 544) -- two factors that tie within that are both right.  Columns beyond d hold level 0;
    padding rows are zero with scale 0.
  * bound: with x~ rebuilt from the tiles, |x - x~| / |x| in fp64 is at most r4max for every row.
  * rows: one huge outlier; all-equal columns, positive and negative (the extreme levels 7 and -8); values exactly on level
    boundaries; denormal elements.
  * an index with a zero row or a NaN row has no usable image, and its searches stay on the 8-bit tiles.
  * dots: the coarse dots a nibble scan keeps differ from the fp64 dots by at most coef_i4 |x||q| on every row, for 8 queries
    (4 perturbed items, 4 fresh draws around the centre -- queries the nibble tiles serve without a rerun, so that the dots read
    back are the nibble scan's; asserted)."""
import os
import sys

import numpy as np
import pytest

from conftest import clustered

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 700, 544           # dp8 = 576: 18 chunks, the last one half padding; 700 rows: 11 tiles, the last one partial


def _sim():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import nibble_sim
    finally:
        sys.path.pop(0)
    return nibble_sim


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_rows():
    rng = np.random.default_rng(31)
    X = clustered(N, D, nclust=8, noise=0.3, seed=31).astype(np.float32).astype(np.float64)
    special = {}
    X[10] = 0.05 * rng.standard_normal(D)
    X[10, 17] = 1.0e3
    special["outlier"] = 10
    X[11] = 0.25
    special["all_equal"] = 11
    X[12] = -0.25
    special["all_equal_negative"] = 12
    X[13] = rng.integers(-7, 8, D).astype(np.float64)      # t = 1 at clip factor 1: every value on a level's lower edge
    X[13, 0] = 7.5
    special["boundaries"] = 13
    X[14, 5:25] = 1.0e-40
    X[14, 30:40] = -1.0e-42
    special["denormals"] = 14
    return np.ascontiguousarray(X), special


def decode(tiles, nrows, ncols):
    """levels [rows][chunks * 32] from [tile][chunk][64 rows][16 bytes]: column 2 j in the low nibble of byte j, 2 j + 1 in the high"""
    t = tiles.astype(np.int16)
    lo, hi = t & 15, t >> 4
    lo, hi = np.where(lo > 7, lo - 16, lo), np.where(hi > 7, hi - 16, hi)
    lv = np.stack([lo, hi], axis=-1).reshape(tiles.shape[0], tiles.shape[1], 64, 32)      # [tile][chunk][row][col]
    lv = lv.transpose(0, 2, 1, 3).reshape(tiles.shape[0] * 64, tiles.shape[1] * 32)
    return lv[:nrows, :ncols]


def test_tiles_scales_and_bound_match_the_numpy_quantiser():
    import pyarrowspace_amd as asp
    sim = _sim()
    X, special = make_rows()
    gp = {"eps": 0.4, "k": 8, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    img = aspace.debug_nibble_image()
    assert img is not None
    tiles, fa4, r4max = img["tiles"], img["fa4"], img["r4max"]
    assert img["chunks"] == 18 and tiles.shape[1:] == (18, 64, 16) and tiles.shape[0] * 64 >= N
    X32 = X.astype(np.float32)
    lv_all = decode(tiles, tiles.shape[0] * 64, 18 * 32)
    assert (lv_all[N:] == 0).all() and (fa4[N:] == 0).all()          # padding rows
    assert (lv_all[:, D:] == 0).all()                                 # padded columns: level 0
    lv_gpu = lv_all[:N, :D]
    m = np.abs(X32).max(axis=1)
    ts = np.stack([(np.float32(f) * m) / np.float32(7.5) for f in sim.CLIPS], axis=1)
    lv_ref, t_ref, best, _ = sim.quantise_rows(X32)
    X64 = X32.astype(np.float64)
    res64 = np.stack([((X64 - (np.clip(np.floor(X32 / ts[:, j:j + 1]), -8, 7).astype(np.float64) + 0.5) * ts[:, j:j + 1].astype(np.float64)) ** 2).sum(1)
                      for j in range(len(sim.CLIPS))], axis=1)
    ties = 0
    for i in range(N):
        js = np.flatnonzero(ts[i] == fa4[i])
        assert len(js) >= 1, (i, fa4[i], ts[i])                       # one of the six steps, bit for bit
        assert res64[i, js[0]] <= res64[i].min() * (1.0 + (D - 1) * 2.0 ** -23), (i, res64[i], js)
        ties += int(fa4[i] != t_ref[i])
        want = lv_ref[i] if fa4[i] == t_ref[i] else np.clip(np.floor(X32[i] / fa4[i]), -8, 7).astype(np.int8)
        assert (lv_gpu[i] == want).all(), (i, np.flatnonzero(lv_gpu[i] != want)[:8])
    print(f"rows whose clip factor differs from numpy's within the rounding of the residual: {ties} of {N}; r4max {r4max}")
    assert ties <= N // 20
    # the special rows
    assert (lv_gpu[special["all_equal"]] == 7).all() and (lv_gpu[special["all_equal_negative"]] == -8).all()
    assert lv_gpu[special["outlier"], 17] == 7
    b = special["boundaries"]
    if fa4[b] == np.float32(1.0):
        assert (lv_gpu[b, 1:] == X[b, 1:].astype(np.int64)).all() and lv_gpu[b, 0] == 7
    assert (lv_gpu[special["denormals"], 5:25] == 0).all() and (lv_gpu[special["denormals"], 30:40] == -1).all()
    # the bound
    xt = (lv_gpu.astype(np.float64) + 0.5) * fa4[:N].astype(np.float64)[:, None]
    r = np.linalg.norm(X64 - xt, axis=1) / np.linalg.norm(X64, axis=1)
    print(f"residual ratio: max {r.max():.4f} (row {int(r.argmax())}), mean {r.mean():.4f}; r4max {r4max:.4f}")
    assert (r <= r4max).all() and r4max <= r.max() * 1.01
    del aspace, gl


@pytest.mark.parametrize("bad", ["zero", "nan"])
def test_a_zero_or_nan_row_leaves_no_image_and_searches_stay_on_8_bits(oracle_lib, bad):
    import pyarrowspace_amd as asp
    n, d = 4096, 512
    X = clustered(n, d, nclust=16, noise=0.3, seed=9)
    X[100] = 0.0 if bad == "zero" else X[100]
    if bad == "nan":
        X[100, 3] = np.nan
    gp = {"eps": 0.4, "k": 10, "topk": 5, "p": 2.0, "sigma": None}
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    assert aspace.debug_nibble_image() is None
    q = _unit(X[7] + 0.001)
    try:
        assert asp._L.as_set_tuning(b"coarse_bits", 4) == 0
        c0 = aspace.search_counters()
        hits = aspace.search(q, gl, 0.62)
        assert aspace.last_scan_bits == 8
        c1 = aspace.search_counters()
    finally:
        assert asp._L.as_set_tuning(b"coarse_bits", -1) == 0
    assert c1["nibble_scans"] == c0["nibble_scans"] and c1["nibble_reruns"] == c0["nibble_reruns"]
    ref = oracle_lib.OracleIndex(X, gp)
    want, lq = ref.search(q, 0.62)
    assert [i for i, _ in hits] == [i for i, _ in want]
    np.testing.assert_allclose([s for _, s in hits], [s for _, s in want], rtol=1e-9)


def test_coarse_dots_lie_within_the_coefficient():
    import pyarrowspace_amd as asp
    from test_gpu_nibble_scan import make_data
    X, gp, qs, _ = make_data(4133, 544, "l2")
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(3)
    d = X.shape[1]
    own = (X @ X[0]) > 0.8
    centre = _unit(X[own].mean(axis=0))
    queries = [_unit(X[i] + 0.02 * rng.standard_normal(d) / np.sqrt(d)) for i in (1, 500, 2000, 4132)]
    queries += [_unit(centre * np.sqrt(d) + 0.3 * rng.standard_normal(d)) * s for s in (1.0, 3.0, 0.25, 1.0)]   # (scaled queries too)
    X64 = X.astype(np.float32).astype(np.float64)
    nx = np.linalg.norm(X64, axis=1)
    try:
        assert asp._L.as_set_tuning(b"coarse_bits", 4) == 0
        for q in queries:
            q = np.ascontiguousarray(q)
            c0 = aspace.search_counters()
            try:
                aspace.search(q, gl, 0.62)
            except asp.PanicException:      # (a scaled query is far from every row in L2: the scan ran all the same)
                assert abs(np.linalg.norm(q) - 1.0) > 0.1
            assert aspace.last_scan_bits == 4
            c1 = aspace.search_counters()
            assert c1["nibble_scans"] == c0["nibble_scans"] + 1 and c1["nibble_reruns"] == c0["nibble_reruns"]
            dots, coef = aspace.debug_last_dots()
            err = np.abs(dots.astype(np.float64) - X64 @ q) / (nx * np.linalg.norm(q))
            print(f"coef_i4 {coef:.4f}, largest |dot - x.q| / (|x||q|) {err.max():.4f}")
            assert 0.05 < coef < 0.2
            assert (err <= coef).all()
    finally:
        assert asp._L.as_set_tuning(b"coarse_bits", -1) == 0
