"""GPU: the feature-mode build stages, one at a time through the staged C ABI (as_space_create_dev, as_feat_gram,
as_feat_graph, as_feat_energy, as_feat_lambdas), on hand-built items, Grams and vectors, against oracle/oracle_np.py
(feature_graph_from_gram, feature_energy).  tests/test_gpu_feature.py covers the same stages end to end on clustered data;
what it cannot reach is here:

  (a) gram_f64_kernel / gram_reduce_kernel on small integers: every entry is an exact integer below 2^53 in any summation
      order, so the Gram is compared bit for bit with numpy's int64 X^T X -- widths below, at and across the 128-column
      tile, both storages, row ranges that are empty, one row, or start and end off the 32-row stage, and 16 421 rows
      (two row splits, the second one short).
  (b) feat_knn_kernel and the CSR on hand-built Grams (the space only supplies D, metric and kernel): a tie run across the
      cut at k and across column 256 (the block's first 256-thread trip), columns with fewer than k passers and with none,
      a key equal to the eps key and one ulp above, k >= D - 1, D = 1 and 2, a zero diagonal, a negative g, and the two
      clamps (g one ulp above sqrt(m_a m_b) under cosine, above m_a = m_b under L2).  Topology exact, values at RTOL; bit
      for bit where two Grams differ by an order-preserving relabelling.  D = 9601 is refused with AS_EUNSUPPORTED.
      D = 9600 itself is NOT computed here: the numpy reference of a 9600 x 9600 Gram needs several GB.
  (c) feat_energy_kernel on vectors whose E and G are known exactly (0, 1.0, 0.5), on row ranges (one call == n one-row
      calls bit for bit: a row's bits do not depend on the slot of the wave's pair that carried it), and on rows of 2401,
      3201 and 4801 features (3, 2 and 1 waves per block; at 4801 x 1101 three trips of the stride loop, the last one
      ending in a lone row).
  (d) the ratio pass of F6 (feat_ratio_pass: T outside 1e-140 .. 1e140): items scaled by 2^+-240 in fp64 storage, with
      2^+-200 as the control that stays on S2 / T^2; and the same branch of q_prepare_feat_kernel for scaled queries.
      Largest relative difference of G between the two routes observed on an MI355X: 5.18e-16 (401 x 130; 4.15e-16 at
      300 x 24), the same at 2^240 and 2^-240; the 2^+-200 controls are bit-identical to the unscaled index.  Scaled
      queries: as_search and as_search_batch return AS_OK for all four scales, lambda_q bit-identical to the unscaled one.

tests/test_feature_stage_inputs.py checks on the CPU that every fixture has the property it is named for."""
import ctypes as C

import numpy as np
import pytest

import feature_stage_ref as fx
from oracle import oracle_np

pytestmark = pytest.mark.gpu

RTOL = 1e-9          # test_gpu_feature.py's
AS_OK, AS_EZEROLAMBDA, AS_EUNSUPPORTED = 0, 2, 4
SENTINEL = -7.25


# ------------------------------------------------------------------------------------------------ the staged C ABI
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _vp(t):
    return C.c_void_p(t.data_ptr())


class Staged:
    """A space (and later a graph) held through the C ABI; freed by close()."""

    def __init__(self, X, gp):
        import torch

        import pyarrowspace_amd as asp
        from pyarrowspace_amd import _lib
        self.torch, self.lib, self.L = torch, _lib, _lib.load()
        self.gp, self.op = asp._parse_graph_params(gp)
        self.n, self.d = X.shape
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda()
        self.sp, self.gr = C.c_void_p(), C.c_void_p()
        st = self.L.as_space_create_dev(_vp(Xd), _lib.DTYPE_F64, self.n, self.d, self.d, C.byref(self.op), C.byref(self.sp))
        assert st == AS_OK, _lib.last_error()

    def gram(self, r0, r1, expect=AS_OK):
        out = self.torch.full((self.d, self.d), float("nan"), dtype=self.torch.float64, device="cuda")
        self.torch.cuda.synchronize()
        assert self.L.as_feat_gram(self.sp, r0, r1, _vp(out)) == expect, self.lib.last_error()
        return out.cpu().numpy()

    def graph(self, gram, expect=AS_OK):
        g = self.torch.from_numpy(np.ascontiguousarray(gram, dtype=np.float64)).cuda()
        self.torch.cuda.synchronize()
        if self.gr:
            self.L.as_free_graph(self.gr)
            self.gr = C.c_void_p()
        st = self.L.as_feat_graph(self.sp, C.byref(self.gp), _vp(g), C.byref(self.gr))
        assert st == expect, (st, self.lib.last_error())
        return st

    def csr(self):
        """(indptr, off-diagonal indices, off-diagonal values, diagonal values): as_graph_csr holds L = D - W with one
        diagonal entry per row."""
        d, nnz = int(self.L.as_nnodes(self.gr)), int(self.L.as_graph_nnz(self.gr))
        ip, ix, v = np.zeros(d + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int64), np.zeros(max(nnz, 1))
        assert self.L.as_graph_csr(self.gr, ip.ctypes.data_as(C.c_void_p), ix.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)) == AS_OK
        assert ip[0] == 0 and ip[d] == nnz
        ix, v = ix[:nnz], v[:nnz]
        rows = np.repeat(np.arange(d), np.diff(ip))
        off = ix != rows
        assert np.array_equal(np.bincount(rows[~off], minlength=d), np.ones(d, dtype=np.int64))
        return np.concatenate([[0], np.cumsum(np.bincount(rows[off], minlength=d))]), ix[off], v[off], v[~off]

    def degrees(self):
        out = np.full(int(self.L.as_nnodes(self.gr)), np.nan)
        assert self.L.as_graph_degrees(self.gr, out.ctypes.data_as(C.c_void_p)) == AS_OK
        return out

    def energy(self, ranges, E=None, G=None):
        """as_feat_energy over each (r0, r1) of `ranges` into sentinel-filled arrays -> (E, G) on the host."""
        t = self.torch
        E = t.full((self.n,), SENTINEL, dtype=t.float64, device="cuda") if E is None else E
        G = t.full((self.n,), SENTINEL, dtype=t.float64, device="cuda") if G is None else G
        t.cuda.synchronize()
        for r0, r1 in ranges:
            assert self.L.as_feat_energy(self.sp, self.gr, r0, r1, _vp(E), _vp(G)) == AS_OK, self.lib.last_error()
        self._EG = (E, G)
        return E.cpu().numpy(), G.cpu().numpy()

    def lambdas(self):
        """as_feat_lambdas on the arrays of the last energy() -> (tau0, lambdas)."""
        E, G = self._EG
        assert self.L.as_feat_lambdas(self.sp, self.gr, _vp(E), _vp(G)) == AS_OK, self.lib.last_error()
        lam = np.empty(self.n)
        assert self.L.as_lambdas(self.sp, lam.ctypes.data_as(C.c_void_p)) == AS_OK
        return float(self.L.as_graph_tau0(self.gr)), lam

    def close(self):
        if self.gr:
            self.L.as_free_graph(self.gr)
        self.L.as_free_space(self.sp)
        self.gr = self.sp = C.c_void_p()


def _reldiff(got, want):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    if got.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    r[got == want] = 0.0
    return float(np.max(r))


def _check_graph(s, ref, label):
    """The staged graph against the oracle's: topology exact, -w, the diagonal and the degrees at RTOL."""
    ip, ix, v, diag = s.csr()
    deg = s.degrees()
    assert np.array_equal(ip, ref["indptr"]), label
    assert np.array_equal(ix, ref["indices"]), label
    print("feature-stage %s: nnz=%d lap=%.3g deg=%.3g" % (label, len(ix), _reldiff(v, ref["lap"]), _reldiff(deg, ref["deg"])))
    np.testing.assert_allclose(v, ref["lap"], rtol=RTOL, atol=0.0, err_msg=label)
    np.testing.assert_allclose(deg, ref["deg"], rtol=RTOL, atol=0.0, err_msg=label)
    assert np.array_equal(_bits(diag), _bits(deg)), label
    return ip, ix, v, deg


def _dummy_items(d, n=3):
    """Items for a space that only has to supply D, metric and kernel: small integers, none of them constant over a row
    (for D > 1), so that the energies over the hand-built graph are not trivially 0."""
    return (np.arange(n * d).reshape(n, d) * 5 % 7).astype(np.float64)


# ------------------------------------------------------------------------------------------------ (a) as_feat_gram
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", fx.GRAM_DS)
def test_gram_of_small_integers_is_exact(d, storage):
    X = fx.gram_items(fx.GRAM_N, d, storage)
    s = Staged(X, fx._gp(1.0, 2, "l2", "gaussian"))
    try:
        got = {r: s.gram(*r) for r in set(fx.GRAM_RANGES + fx.GRAM_SPLIT)}
    finally:
        s.close()
    for (r0, r1), g in got.items():
        assert np.array_equal(_bits(g), _bits(g.T)), (r0, r1)                    # gram[a][b] and gram[b][a]: the same bits
        assert np.array_equal(_bits(g), _bits(fx.int_gram_of(X, r0, r1))), (r0, r1)
    assert not got[(0, 0)].any()
    assert np.array_equal(_bits(sum(got[r] for r in fx.GRAM_SPLIT)), _bits(got[(0, fx.GRAM_N)]))


def test_gram_over_two_row_splits_is_exact():
    n, d = fx.GRAM_BIG
    X = fx.gram_items(n, d, "f32")
    s = Staged(X, fx._gp(1.0, 2, "l2", "gaussian"))
    try:
        whole, tail = s.gram(0, n), s.gram(7, n)
    finally:
        s.close()
    assert np.array_equal(_bits(whole), _bits(fx.int_gram_of(X, 0, n))) and np.array_equal(_bits(whole), _bits(whole.T))
    assert np.array_equal(_bits(tail), _bits(fx.int_gram_of(X, 7, n))) and np.array_equal(_bits(tail), _bits(tail.T))


# ------------------------------------------------------------------------------------------------ (b) as_feat_graph
@pytest.mark.parametrize("name", sorted(fx.GRAM_FIXTURES))
def test_graph_of_a_hand_built_gram(name):
    gram, gp = fx.GRAM_FIXTURES[name]()
    d = gram.shape[0]
    ref = fx.expected_graph(name)
    X = _dummy_items(d)
    s = Staged(X, gp)
    try:
        s.graph(gram)
        ip, ix, v, deg = _check_graph(s, ref, name)
        E, G = s.energy([(0, X.shape[0])])
    finally:
        s.close()
    Er, Gr = oracle_np.feature_energy(ref, X)
    np.testing.assert_allclose(E, Er, rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(G, Gr, rtol=RTOL, atol=0.0)
    if name == "d1":
        assert len(ix) == 0 and deg.tolist() == [0.0] and not E.any() and not G.any()
    if name == "d2":
        assert ix.tolist() == [1, 0]
    if name == "kclamp":
        assert np.diff(ip).tolist() == [d - 1] * d                     # k = 50 clamped to D - 1: the complete graph
    if name == "l2_clamp":
        assert ix[ip[0] : ip[1]].tolist() == [1, 2] and v[ip[0]] == -1.0          # key clamped to 0: dist 0, weight kernel(0) = 1
    if name.startswith("cosine"):
        assert ix[ip[0] : ip[1]][:2].tolist() == [1, 2] and v[ip[0]] == -1.0 and v[ip[0] + 1] == -1.0   # c > 1: distance 0
        assert (ip[5] - ip[4], ip[6] - ip[5]) == ((2, 2) if name == "cosine_eps1" else (0, 0))


def test_tie_run_across_the_cut_and_the_first_trip():
    """The hub's list: 11, 12, then the first four of seven columns at one key, two of them below column 256 and two above."""
    gram, gp = fx.tie_fixture()
    ref = fx.expected_graph("tie")
    s = Staged(_dummy_items(fx.TIE_D), gp)
    try:
        s.graph(gram)
        ip, ix, v, _ = s.csr()
        deg = s.degrees()
    finally:
        s.close()
    hub = ix[ip[fx.TIE_HUB] : ip[fx.TIE_HUB + 1]].tolist()
    assert hub == sorted([11, 12] + list(fx.TIE_MEMBERS[:4])) == ref["indices"][ref["indptr"][fx.TIE_HUB] : ref["indptr"][fx.TIE_HUB + 1]].tolist()
    for c in fx.TIE_PAIR:
        assert ip[c + 1] - ip[c] == 1
    assert (np.diff(ip) == 0).sum() == (np.diff(ref["indptr"]) == 0).sum() > 100 and (deg[np.diff(ip) == 0] == 0.0).all()


def test_order_preserving_relabelling_changes_no_bit():
    """One more lonely column at index 7 moves every later label up by one (other columns fall into the block's second
    trip) and keeps every order: the same graph, bit for bit."""
    gram, gp = fx.tie_fixture()
    big, _, keep = fx.tie_fixture_shifted()
    outs = []
    for g in (gram, big):
        s = Staged(_dummy_items(g.shape[0]), gp)
        try:
            s.graph(g)
            outs.append(s.csr() + (s.degrees(),))
        finally:
            s.close()
    (ip0, ix0, v0, dg0, deg0), (ip1, ix1, v1, dg1, deg1) = outs
    assert np.array_equal(np.diff(ip0), np.diff(ip1)[keep]) and ip1[8] == ip1[7]
    assert np.array_equal(keep[ix0], ix1)
    assert np.array_equal(_bits(v0), _bits(v1)) and np.array_equal(_bits(deg0), _bits(deg1[keep])) and np.array_equal(_bits(dg0), _bits(dg1[keep]))


def test_more_than_9600_features_are_refused():
    """2 x 8 x D bytes of LDS per block: D = 9601 -> AS_EUNSUPPORTED before anything is launched (the Gram pointer is a
    dummy of 8 bytes: nothing may read it)."""
    import torch
    d = 9601
    s = Staged(np.ones((1, d)), fx._gp(1.0, 2, "l2", "gaussian"))
    try:
        dummy = torch.zeros(1, dtype=torch.float64, device="cuda")
        st = s.L.as_feat_graph(s.sp, C.byref(s.gp), _vp(dummy), C.byref(s.gr))
        assert st == AS_EUNSUPPORTED and not s.gr and "9600" in s.lib.last_error()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ (c) as_feat_energy
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_energy_of_vectors_with_known_dispersion(storage):
    gram, gp = fx.path_fixture()
    X, g_want = fx.path_vectors(storage)
    ref = oracle_np.feature_graph_from_gram(gram, oracle_np.resolve_params(gp))
    s = Staged(X, gp)
    try:
        s.graph(gram)
        _check_graph(s, ref, "path")
        E, G = s.energy([(0, X.shape[0])])
    finally:
        s.close()
    assert np.array_equal(_bits(G), _bits(g_want))                    # 0, 0, 1.0, 1.0, 0.5, 0.5: exact
    assert E[0] == 0.0 and E[1] == 0.0
    np.testing.assert_allclose(E, oracle_np.feature_energy(ref, X)[0], rtol=RTOL, atol=0.0)


def test_energy_row_ranges_change_no_bit():
    """37 rows.  One call over [0, n) == n one-row calls == calls over odd starts, odd lengths and empty ranges, bit for
    bit; positions outside a call's range keep the sentinel."""
    X, gram, gp = fx.range_fixture()
    n = fx.RANGE_N
    ref = oracle_np.feature_graph_from_gram(gram, oracle_np.resolve_params(gp))
    assert len(ref["ea"]) > 64                                       # more than one edge per lane
    s = Staged(X, gp)
    try:
        s.graph(gram)
        _check_graph(s, ref, "range")
        whole = s.energy([(0, n)])
        single = s.energy([(r, r + 1) for r in range(n)])
        odd = s.energy([(0, 0), (0, 1), (1, 4), (4, 4), (4, 9), (9, 10), (10, 33), (33, 36), (36, 37), (37, 37)])
        part = s.energy([(5, 5), (7, 20), (21, 22)])
    finally:
        s.close()
    Er, Gr = oracle_np.feature_energy(ref, X)
    print("feature-stage range: E=%.3g G=%.3g" % (_reldiff(whole[0], Er), _reldiff(whole[1], Gr)))
    np.testing.assert_allclose(whole[0], Er, rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(whole[1], Gr, rtol=RTOL, atol=0.0)
    for other in (single, odd):
        assert np.array_equal(_bits(other[0]), _bits(whole[0])) and np.array_equal(_bits(other[1]), _bits(whole[1]))
    inside = np.zeros(n, dtype=bool)
    inside[7:20] = inside[21] = True
    for a, w in zip(part, whole):
        assert np.array_equal(_bits(a[inside]), _bits(w[inside])) and (a[~inside] == SENTINEL).all()


@pytest.mark.parametrize("n,d", fx.WIDE_SHAPES)
def test_energy_of_wide_rows(n, d):
    """2401, 3201 and 4801 features: 16 d bytes of LDS per wave leave room for 3, 2 and 1 waves in 150 KiB, one block per
    CU; at 4801 features a block carries two rows, so 1101 rows take three trips on a device of 256 CUs and the last trip
    ends in a lone row.  (feat_knn_kernel needs 2 x 8 x 4801 bytes > 64 KiB of dynamic LDS there.)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves, grid, trips, tail = fx.energy_launch(d, n, cus)
    assert waves == {2401: 3, 3201: 2, 4801: 1}[d]
    if d == 4801:
        assert cus * 2 * waves < n and trips == 3 and tail % 2 == 1, (cus, waves, grid, trips, tail)
    X, gram, gp = fx.wide_fixture(n, d)
    ref = oracle_np.feature_graph_from_gram(gram, oracle_np.resolve_params(gp))
    s = Staged(X, gp)
    try:
        s.graph(gram)
        _check_graph(s, ref, "wide%d" % d)
        E, G = s.energy([(0, n)])
    finally:
        s.close()
    Er, Gr = oracle_np.feature_energy(ref, X)
    print("feature-stage wide %dx%d: waves=%d grid=%d trips=%d tail=%d E=%.3g G=%.3g" % (n, d, waves, grid, trips, tail, _reldiff(E, Er), _reldiff(G, Gr)))
    np.testing.assert_allclose(E, Er, rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(G, Gr, rtol=RTOL, atol=0.0)


# ------------------------------------------------------------------------------------------------ (d) the ratio pass
def _staged_index(X, gp):
    n = X.shape[0]
    s = Staged(X, gp)
    try:
        s.graph(s.gram(0, n))
        ip, ix, v, diag = s.csr()
        E, G = s.energy([(0, n)])
        tau0, lam = s.lambdas()
        return dict(indptr=ip, indices=ix, lap=v, deg=s.degrees(), E=E, G=G, tau0=tau0, lambdas=lam)
    finally:
        s.close()


@pytest.mark.parametrize("n,d,k", fx.SCALED_SHAPES)
def test_ratio_pass_on_scaled_items(n, d, k):
    """Items times 2^+-240 put every T beyond 1e+-140 (feat_ratio_pass), times 2^+-200 leave it inside (S2 / T^2).  The
    scaling is exact: topology, weights, E and tau0 are the unscaled index's bit for bit; G and lambda at RTOL."""
    X, gp = fx.scaled_base(n, d, k)
    ref = fx.scaled_oracle(n, d, k, 0)
    base = _staged_index(X, gp)
    assert np.array_equal(base["indices"], ref["indices"])
    worst = 0.0
    for sc in fx.RATIO_SCALES + fx.CONTROL_SCALES:
        got = _staged_index(np.ldexp(X, sc), gp)
        for key in ("indptr", "indices"):
            assert np.array_equal(got[key], base[key]), (sc, key)
        for key in ("lap", "deg", "E"):
            assert np.array_equal(_bits(got[key]), _bits(base[key])), (sc, key)
        assert got["tau0"] == base["tau0"]
        dg = _reldiff(got["G"], base["G"])
        print("feature-stage ratio %dx%d scale 2^%d: G vs unscaled=%.3g G vs oracle=%.3g lambda vs oracle=%.3g"
              % (n, d, sc, dg, _reldiff(got["G"], ref["G"]), _reldiff(got["lambdas"], ref["lambdas"])))
        if sc in fx.RATIO_SCALES:
            worst = max(worst, dg)
        else:
            assert dg == 0.0                                           # the control stays on S2 / T^2: exact scaling again
        for other in (base, ref):
            np.testing.assert_allclose(got["G"], other["G"], rtol=RTOL, atol=0.0)
            np.testing.assert_allclose(got["lambdas"], other["lambdas"], rtol=RTOL, atol=0.0)
        np.testing.assert_allclose(got["E"], ref["E"], rtol=RTOL, atol=0.0)
    print("feature-stage ratio %dx%d: largest relative difference of G between S2/T^2 and the ratio pass = %.3g" % (n, d, worst))


def _search_status(aspace, gl, q):
    """as_search at tau = 1 -> (status, lambda_q)."""
    from pyarrowspace_amd import _lib
    L = _lib.load()
    topk = max(min(int(gl.graph_params["topk"]), aspace.nitems), 1)
    idx, sc = np.empty(topk, dtype=np.int64), np.empty(topk)
    ln, lq = C.c_int64(0), C.c_double(0.0)
    st = L.as_search(aspace._h, gl._h, q.ctypes.data_as(C.c_void_p), q.shape[0], 1.0, idx.ctypes.data_as(C.c_void_p),
                     sc.ctypes.data_as(C.c_void_p), C.byref(ln), C.byref(lq))
    return st, float(lq.value)


def _batch_status(aspace, gl, Q):
    """as_search_batch at tau = 1 -> (status, per-query status, lambda_q)."""
    from pyarrowspace_amd import _lib
    L = _lib.load()
    b, topk = Q.shape[0], max(min(int(gl.graph_params["topk"]), aspace.nitems), 1)
    idx, sc = np.empty((b, topk), dtype=np.int64), np.empty((b, topk))
    ln, lq, stt = np.zeros(b, dtype=np.int64), np.zeros(b), np.zeros(b, dtype=np.int32)
    st = L.as_search_batch(aspace._h, gl._h, Q.ctypes.data_as(C.c_void_p), b, Q.shape[1], 1.0, idx.ctypes.data_as(C.c_void_p),
                           sc.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), lq.ctypes.data_as(C.c_void_p),
                           stt.ctypes.data_as(C.c_void_p))
    return st, stt, lq


@pytest.mark.parametrize("sc", fx.RATIO_SCALES + fx.CONTROL_SCALES)
def test_ratio_pass_on_scaled_queries(sc):
    """The same branch in q_prepare_feat_kernel, on an ordinary index: lambda_q of q 2^s against lambda_q of q and the
    oracle's, from as_search and from as_search_batch at B = 3 (slots in blockIdx.z).  Only lambda_q is asserted: what the
    scan makes of a query whose fp32 copy is 0 or inf is not this test's subject."""
    import pyarrowspace_amd as asp
    n, d, k = fx.SCALED_SHAPES[0]
    X, gp = fx.scaled_base(n, d, k)
    ref = fx.scaled_oracle(n, d, k, 0)
    aspace, gl = asp.ArrowSpaceBuilder.build(gp, X)
    rng = np.random.default_rng(5)
    Q = np.stack([X[i] + 0.05 * rng.standard_normal(d) / np.sqrt(d) for i in (7, 100, 250)])
    want = np.array([oracle_np.query_lambda(ref, q) for q in Q])
    plain = np.array([aspace.query_lambda(np.ascontiguousarray(q), gl) for q in Q])
    np.testing.assert_allclose(plain, want, rtol=RTOL, atol=0.0)
    Qs = np.ascontiguousarray(np.ldexp(Q, sc))
    T = fx.edge_energy_sums(ref, Qs)                                   # (the weights do not move with the items' scale)
    assert ((T > 1e140) | (T < 1e-140)).all() if sc in fx.RATIO_SCALES else ((T > 1e-140) & (T < 1e140)).all()
    for b in range(3):
        st, lq = _search_status(aspace, gl, np.ascontiguousarray(Qs[b]))
        print("feature-stage query 2^%d slot %d: as_search status=%d lambda_q=%.17g (unscaled %.17g)" % (sc, b, st, lq, plain[b]))
        assert st == AS_OK
        assert abs(lq - plain[b]) <= RTOL * plain[b] and abs(lq - want[b]) <= RTOL * want[b]
    st, stt, lq = _batch_status(aspace, gl, Qs)
    print("feature-stage query 2^%d batch: status=%d per-query=%s reldiff=%.3g" % (sc, st, stt.tolist(), _reldiff(lq, plain)))
    assert st == AS_OK and (stt == AS_OK).all()
    np.testing.assert_allclose(lq, plain, rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(lq, want, rtol=RTOL, atol=0.0)


def test_feature_power_of_two_scaling_changes_nothing():
    """The feature-mode twin of test_gpu_edges.py's test_power_of_two_scaling_changes_nothing: fp32 storage, cosine, items
    times 2^+-40 -- graph, E, G and lambdas bit-identical (everything on S2 / T^2, every step scaled exactly)."""
    n, d, k = 300, 24, 5
    X, gp = fx.scaled_base(n, d, k)
    X = X.astype(np.float32).astype(np.float64)
    base = _staged_index(X, gp)
    assert len(base["indices"]) > 0 and (base["lambdas"] > 0).all()
    for sc in (40, -40):
        Xs = np.ldexp(X, sc)
        assert np.array_equal(Xs.astype(np.float32).astype(np.float64), Xs)
        got = _staged_index(Xs, gp)
        for key in ("indptr", "indices"):
            assert np.array_equal(got[key], base[key]), (sc, key)
        for key in ("lap", "deg", "E", "G", "lambdas"):
            assert np.array_equal(_bits(got[key]), _bits(base[key])), (sc, key)
        assert got["tau0"] == base["tau0"]
