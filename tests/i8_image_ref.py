"""The rows that tests/test_i8_image_inputs.py (numpy only) and tests/test_gpu_i8_image.py (the image read back from the device) put
through the int8 two-digit quantiser, and what both read off the reference (tools/i8_sim.py).

Row sets, each `clustered` rows with the special rows written over some of them:

  * "d40", "d96", "d544", "d1056": 700 rows (as the nibble image test: 11 tiles of 64, the last partial; 3 row tiles with padding
    rows) at d = 40 (dp8 = 64), 96 (dp8 = 128: half the last slab is padding), 544 (dp8 = 576) and 1056 (dp8 = 1088: beyond the
    1040 columns up to which the integer sums are exact floats), with all the special rows;
  * "trips": 8300 x 40.  The quantiser's grid is capped at 2048 blocks of 4 waves, a wave per row: rows from 8192 on are the
    waves' SECOND trips.  The row with the largest U is row 8250, the row with the largest V the last one;
  * "trips_early": the same rows with those two at rows 100 and 50 -- first trips of waves that go on to a second one (rows 8292
    and 8242, plain clustered rows), so a maximum that a later trip overwrites is lost.

Special rows (every value exactly an fp32; s = max|x| of the row):

  outlier        1e3 among 0.05 noise
  all_equal      all 0.25; all_equal_negative: all -0.25 (every q = +-16256: a1 = +-127, a2 = 0)
  a2_max         s = 127/128, so that 16256 / s = 16384 and x = q / 16384 quantises to exactly q: every q but the largest
                 = 63 (mod 128), a2 = 63
  a2_min         likewise, every q but the largest = -64 (mod 128), a2 = -64
  half_ties      likewise, x = (j + 1/2) / 16384: every 16256 x / s but the largest lies exactly on .5, q = the even neighbour
  single_spike   one nonzero element
  zero           all zero: digits 0, scale 0, not counted in the maxima
  denormals      elements of 1e-40 and -1e-42 in a clustered row
  spike_noise    a spike of 1 and +-0.4 / 16256 everywhere else: everything but the spike rounds to 0 with residue 0.4 -- the
                 largest U of all, growing like sqrt(d): the handle for the 1e-3 gate (under it at d = 40 and 96, over at 544, 1056)

No row's squared norm leaves [2^-100, 2^120] (beyond it the whole index runs in fp64 and the image is out of its contract)."""
import functools
import os
import sys

import numpy as np

from conftest import clustered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 700
DIMS = {"d40": 40, "d96": 96, "d544": 544, "d1056": 1056}
SETS = ("d40", "d96", "d544", "d1056", "trips", "trips_early")
GATE_INT8 = {"d40": True, "d96": True, "d544": False, "d1056": False, "trips": True, "trips_early": True}   # coefficient under 1e-3
TRIP = 8192            # rows per trip of the quantiser's grid-stride loop: 2048 blocks x 4 waves
ROW_TILE = 256


def sim():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import i8_sim
    finally:
        sys.path.pop(0)
    return i8_sim


def _spike_noise(d, rng):
    v = np.where(rng.integers(0, 2, d) == 1, 1.0, -1.0) * float(np.float32(0.4 / 16256.0))
    v[3] = 1.0
    return v


def _from_q(q):
    """s = 127/128: the row x = q / 16384 with q[0] = 16256 quantises to exactly q"""
    q = q.astype(np.float64)
    q[0] = 16256.0
    return q / 16384.0


def special_rows(d, rng, base):
    """name -> row; `base`: a clustered row for the denormals to sit in"""
    rows = {}
    v = 0.05 * rng.standard_normal(d)
    v[17] = 1.0e3
    rows["outlier"] = v
    rows["all_equal"] = np.full(d, 0.25)
    rows["all_equal_negative"] = np.full(d, -0.25)
    rows["a2_max"] = _from_q(128 * rng.integers(-100, 100, d) + 63)
    rows["a2_min"] = _from_q(128 * rng.integers(-100, 101, d) - 64)
    rows["half_ties"] = _from_q(rng.integers(-16000, 16000, d) + 0.5)
    v = np.zeros(d)
    v[5] = 3.0
    rows["single_spike"] = v
    rows["zero"] = np.zeros(d)
    v = base.copy()
    v[5:25] = 1.0e-40
    v[30:40] = -1.0e-42
    rows["denormals"] = v
    rows["spike_noise"] = _spike_noise(d, rng)
    return rows


@functools.lru_cache(maxsize=None)
def make_set(name):
    """-> (X float64 [n, d], every value an fp32, read-only; {special row's name: its index})"""
    special = {}
    if name in DIMS:
        d = DIMS[name]
        rng = np.random.default_rng(1000 + d)
        X = clustered(N, d, nclust=8, noise=0.3, seed=31 + d)
        for t, (key, row) in enumerate(special_rows(d, rng, X[10]).items()):
            X[10 + 7 * t] = row
            special[key] = 10 + 7 * t
    else:
        d = 40
        rng = np.random.default_rng(77)
        X = clustered(8300, d, nclust=16, noise=0.3, seed=77)
        iu, iv = (8250, 8299) if name == "trips" else (100, 50)
        X[iu] = _spike_noise(d, rng)
        # the largest V: a2 = 63 on every column but the largest, |q| between 20 and 50 high digits
        k = rng.integers(20, 51, d) * np.where(rng.integers(0, 2, d) == 1, 1, -1)
        X[iv] = _from_q(128 * k + 63)
        special = {"spike_noise": iu, "v_max": iv}
    X = np.ascontiguousarray(X.astype(np.float32).astype(np.float64))
    X.setflags(write=False)
    return X, special


@functools.lru_cache(maxsize=None)
def reference(name):
    """the numpy quantiser's answer for a row set (computed once, shared, not to be changed)"""
    X, _ = make_set(name)
    return sim().quantise_rows(X.astype(np.float32))


def digits_of_image(x8):
    """int8 [rows][slab][2][64] -> (a1, a2) int8 [rows][slab * 64]: bytes 0-63 of a 128-byte slab row are a1, bytes 64-127 a2"""
    rows = x8.shape[0]
    return np.ascontiguousarray(x8[:, :, 0, :]).reshape(rows, -1), np.ascontiguousarray(x8[:, :, 1, :]).reshape(rows, -1)


def tiles_of_digits(a1):
    """the high digits [rows][dp8] (rows a multiple of 64) -> [tile][chunk][64 rows][16 bytes]: (row, c) at [row // 64][c // 16][row % 64][c % 16]"""
    rows, dp8 = a1.shape
    return np.ascontiguousarray(a1.reshape(rows // 64, 64, dp8 // 16, 16).transpose(0, 2, 1, 3))
