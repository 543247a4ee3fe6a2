"""No GPU: the rows of tests/test_gpu_i8_image.py (tests/i8_image_ref.py) put through the numpy quantiser (tools/i8_sim.py) do what
that test relies on.

  * the special rows hit their edges: the a2 extremes, the half ties (round half to even), the saturated digits, the zero row
    outside the maxima, the denormals rounding to 0, everything but the spike of the spike-plus-noise row rounding to 0;
  * the row with the largest U is the spike-plus-noise row in every set; in "trips" it and the row with the largest V (the last
    one) are second trips of the quantiser's grid-stride loop, in "trips_early" first trips of waves that go on to a second one;
  * the bound is satisfiable: over every pair of rows of a set the true error of the three kept integer products is at most
    oracle_np.ring_coef_i8(U, V) |x_i||x_j| with the simulated maxima (so a correct image passes the GPU test with room);
  * the simulated coefficient of every set is at least 10 % away from the 1e-3 gate, on the side the GPU test asserts;
  * the simulated maxima themselves lie inside the limits the GPU test holds the device's to."""
import numpy as np
import pytest

import i8_image_ref as ref
from oracle import oracle_np


@pytest.mark.parametrize("name", list(ref.DIMS))
def test_special_rows_hit_their_edges(name):
    X, special = ref.make_set(name)
    r = ref.reference(name)
    d = X.shape[1]
    a1, a2, q = r["a1"].astype(np.int64), r["a2"].astype(np.int64), r["q"].astype(np.int64)
    assert a1.shape[1] == (d + 63) // 64 * 64 and (128 * a1 + a2 == q).all()
    assert (q[:, d:] == 0).all()
    n64 = (X * X).sum(axis=1)
    live = n64 > 0
    assert (n64[live] >= 2.0 ** -100).all() and (n64 <= 2.0 ** 120).all()          # inside the safe band
    i = special["a2_max"]
    assert (a2[i, 1:d] == 63).all() and q[i, 0] == 16256 and (q[i, :d] == np.rint(X[i] * 16384.0)).all()
    i = special["a2_min"]
    assert (a2[i, 1:d] == -64).all() and q[i, 0] == 16256 and (q[i, :d] == np.rint(X[i] * 16384.0)).all()
    i = special["half_ties"]
    sc = X[i] * 16384.0
    assert (np.abs(sc[1:] - np.floor(sc[1:])) == 0.5).all()                       # exactly on .5 ...
    assert (q[i, 1:d] % 2 == 0).all() and (np.abs(q[i, 1:d] - sc[1:]) == 0.5).all()   # ... and rounded to the even neighbour
    assert (np.floor(sc[1:]) % 2 == 0).any() and (np.floor(sc[1:]) % 2 == 1).any()    # both directions occur
    assert (a1[special["all_equal"], :d] == 127).all() and (a2[special["all_equal"]] == 0).all()
    assert (a1[special["all_equal_negative"], :d] == -127).all() and (a2[special["all_equal_negative"]] == 0).all()
    i = special["single_spike"]
    assert q[i, 5] == 16256 and np.count_nonzero(q[i]) == 1 and r["v_true"][i] == 0.0
    i = special["zero"]
    assert not q[i].any() and r["fa8"][i] == 0.0 and r["u_est"][i] == 0.0 and r["v_est"][i] == 0.0 and r["u_true"][i] == 0.0
    i = special["denormals"]
    assert (X[i, 5:25] > 0).all() and (X[i, 5:25] < 2.0 ** -126).all() and (X[i, 30:40] < 0).all()
    assert not q[i, 5:25].any() and not q[i, 30:40].any()
    i = special["spike_noise"]
    assert q[i, 3] == 16256 and np.count_nonzero(q[i]) == 1
    assert q[special["outlier"], 17] == 16256


@pytest.mark.parametrize("name", ref.SETS)
def test_which_rows_hold_the_maxima(name):
    X, special = ref.make_set(name)
    r = ref.reference(name)
    n = X.shape[0]
    iu = special["spike_noise"]
    assert int(r["u_true"].argmax()) == iu and int(r["u_est"].argmax()) == iu
    # (a lost row must show: the runner-up lies clearly below, further than the limits of the GPU test are wide)
    assert np.sort(r["u_true"])[-2] < 0.8 * r["U_true"]
    if name.startswith("trips"):
        iv = special["v_max"]
        assert int(r["v_true"].argmax()) == iv and int(r["v_est"].argmax()) == iv
        assert np.sort(r["v_true"])[-2] < 0.97 * r["V_true"]
        rows_alloc = (n + ref.ROW_TILE - 1) // ref.ROW_TILE * ref.ROW_TILE + ref.ROW_TILE
        assert ref.TRIP < n < rows_alloc < 2 * ref.TRIP                  # two trips, the second partial
        if name == "trips":
            assert iu >= ref.TRIP and iv == n - 1
        else:
            # first trips of waves whose second trip is a real row with smaller values
            assert max(iu, iv) + ref.TRIP < n and iu != iv


@pytest.mark.parametrize("name", ref.SETS)
def test_every_pair_lies_within_the_coefficient_and_the_gate_is_clear(name):
    X, special = ref.make_set(name)
    r = ref.reference(name)
    sim = ref.sim()
    coef = oracle_np.ring_coef_i8(r["U_est"], r["V_est"])
    assert coef == sim.coef_i8(r["U_est"], r["V_est"])
    worst, at, dead = sim.pair_errors(X.astype(np.float32), r["a1"], r["a2"], r["fa8"])
    print(f"{name}: U {r['U_est']:.4e} (true {r['U_true']:.4e}), V {r['V_est']:.4e} (true {r['V_true']:.4e}), coefficient {coef:.3e}, "
          f"largest pair error {worst:.3e} = {worst / coef:.3f} coef at {at}")
    assert worst <= coef and dead == 0.0
    # the gate: 1e-3, with 10 % of room on the side the GPU test asserts
    assert (coef < 0.9e-3) if ref.GATE_INT8[name] else (coef > 1.1e-3)
    # what the GPU test holds the device's maxima to (its docstring derives the limits)
    dp8 = r["a1"].shape[1]
    rnd = 1.0 + dp8 * 2.0 ** -24
    assert r["U_true"] <= r["U_est"] <= (r["U_true"] + 0.004 * np.sqrt(dp8) * r["ratio"].max()) * 1.001 * rnd
    assert r["V_true"] <= r["V_est"] <= r["V_true"] * 1.001 * rnd
