"""Hand-built inputs of the feature-mode stage tests (tests/test_gpu_feature_stage.py runs them on the GPU,
tests/test_feature_stage_inputs.py checks on the CPU that each one has the property it is named for).  No GPU, no torch:
numpy and oracle/oracle_np.py only.  Every builder is cached and its arrays are never written to.

A "Gram fixture" is (gram fp64 [D][D], graph_params): as_feat_graph takes whatever symmetric array it is handed, so most of
them are not the Gram of any item matrix.  The L2 ones are integer Grams G = F F^T of virtual integer columns (row a of F is
column a's vector): every key m_a + m_b - 2 g_ab is an exact integer on any machine, so equal keys are equal bits."""
import functools

import numpy as np

from conftest import calibrate_feature_eps, clustered
from oracle import oracle_np

ULP1 = 1.0 + 2.0 ** -52


def _gp(eps, k, metric, kernel, sigma=None):
    return {"eps": float(eps), "k": int(k), "topk": 3, "p": 2.0, "sigma": sigma, "metric": metric, "kernel": kernel,
            "lambda_mode": "feature"}


def _int_gram(F):
    F = np.asarray(F, dtype=np.int64)
    G = F @ F.T
    assert np.abs(G).max() < 2 ** 50
    return G.astype(np.float64)


def keys_of(gram, prm):
    """F2's key matrix, the oracle's arithmetic."""
    m = np.diagonal(gram)
    if prm["metric"] == oracle_np.METRIC_COSINE:
        den = np.sqrt(np.outer(m, m))
        c = np.where(den > 0, gram / np.where(den > 0, den, 1.0), 0.0)
        return 1.0 - np.minimum(1.0, np.maximum(0.0, c))
    return np.maximum(0.0, m[:, None] + m[None, :] - 2.0 * gram)


# ------------------------------------------------------------------------------------------------ F3: ties and the cut
TIE_D, TIE_K, TIE_HUB = 300, 6, 10
TIE_MEMBERS = (254, 255, 256, 257, 258, 290, 299)     # all at key 25 from the hub; the list takes the first four
TIE_PAIR = (20, 21)                                   # two columns that pass for each other alone: cnt = 1 < k


@functools.lru_cache(maxsize=None)
def tie_fixture():
    """D = 300, L2 / gaussian, eps^2 = 30.25, k = 6.  One axis per column.  The hub (column 10) is the origin; 11 and 12
    sit at keys 1 and 4 from it; the seven members sit at 5 on an axis of their own: key 25 from the hub, 50 from one
    another.  Each member has six satellites at key 1 (2 among themselves, 26 from the hub), so a member's own list is
    full before the hub's turn: the edges hub - member exist through the hub's list alone, and which four of the seven it
    takes is visible in the CSR.  20 and 21 share a far axis (key 1 to each other, nothing else passes); every other column
    is alone on a far axis and lists nothing."""
    D = TIE_D
    F = np.zeros((D, D), dtype=np.int64)
    F[11, 11], F[12, 12] = 1, 2
    used = {TIE_HUB, 11, 12, *TIE_MEMBERS, *TIE_PAIR}
    free = [c for c in range(D) if c not in used]
    for t in TIE_MEMBERS:
        F[t, t] = 5
        for _ in range(TIE_K):
            s = free.pop(len(free) // 2)              # from the middle outwards: satellites on both sides of column 256
            F[s, t], F[s, s] = 5, 1
    p1, p2 = TIE_PAIR
    F[p1, p1], F[p2, p1], F[p2, p2] = 1000, 1000, 1
    for c in free:
        F[c, c] = 100
    return _int_gram(F), _gp(5.5, TIE_K, "l2", "gaussian")


@functools.lru_cache(maxsize=None)
def tie_fixture_shifted(at=7):
    """tie_fixture with one more lonely column inserted at index `at`: every label from `at` on moves up by one (255 -> 256:
    other columns fall into the block's second trip), no order between two columns changes."""
    gram, gp = tie_fixture()
    D = gram.shape[0]
    keep = np.array([c for c in range(D + 1) if c != at])
    out = np.zeros((D + 1, D + 1))
    out[np.ix_(keep, keep)] = gram
    out[at, at] = 100.0 ** 2
    return out, gp, keep


# ------------------------------------------------------------------------------------------------ F3: the eps line
@functools.lru_cache(maxsize=None)
def eps_fixture():
    """D = 5, L2.  Column 0 is the origin and every off-diagonal entry is 0: key(0, b) = m_b exactly.  m_1 = eps * eps
    (in), m_2 = one ulp above (out), m_3 = half of it (in), m_4 = four times (out).  Between two other columns the key is
    m_a + m_b > eps^2."""
    eps = 0.3
    ek = eps * eps
    m = np.array([0.0, ek, np.nextafter(ek, np.inf), 0.5 * ek, 4.0 * ek])
    return np.diag(m), _gp(eps, 3, "l2", "rational")


# ------------------------------------------------------------------------------------------------ small shapes
@functools.lru_cache(maxsize=None)
def d1_fixture():
    return np.array([[4.0]]), _gp(1.0, 3, "l2", "gaussian")


@functools.lru_cache(maxsize=None)
def d2_fixture():
    """D = 2, k = 1: one edge of key 1."""
    return _int_gram([[0], [1]]), _gp(1.5, 1, "l2", "gaussian")


@functools.lru_cache(maxsize=None)
def kclamp_fixture():
    """D = 6, k = 50 >= D - 1, eps beyond every key: the complete graph, lists of D - 1."""
    F = np.random.default_rng(3).integers(-3, 4, (6, 3))
    F[0] = (0, 0, 0)
    F[1] = (1, 0, 0)
    assert len({tuple(r) for r in F.tolist()}) == 6
    return _int_gram(F), _gp(20.0, 50, "l2", "rational", sigma=3.0)


@functools.lru_cache(maxsize=None)
def l2_clamp_fixture():
    """D = 3, m = (4, 4, 9).  g_01 is one ulp above m_0 = m_1: m_0 + m_1 - 2 g_01 < 0 -> key 0, dist 0, weight kernel(0) = 1."""
    g = np.array([[4.0, 4.0 * ULP1, 5.0], [4.0 * ULP1, 4.0, 5.0], [5.0, 5.0, 9.0]])
    return g, _gp(2.0, 2, "l2", "gaussian")


@functools.lru_cache(maxsize=None)
def cosine_fixture(eps):
    """D = 8, cosine / rational, k = 2, unit diagonal but for column 5.
      0, 1 duplicates (g = 1); g_02 one ulp above sqrt(m_0 m_2) = 1: c > 1 -> distance 0, so 0 lists 1 then 2 by index;
      3 at cosine 0.5 from 0, 1, 2 (a tie run of three, the cut inside);
      4 has a negative g with everything: rectified to distance 1;
      5 has a zero diagonal: c = 0, distance 1 to everything;
      6, 7 at cosine 0.75 from each other and 0.25 from 0..3.
    eps = 1.0: columns 4 and 5 list 0 and 1 (key == eps, ties by index); eps = 0.9: they list nothing."""
    g = np.zeros((8, 8))
    for a, b, v in [(0, 1, 1.0), (0, 2, ULP1), (1, 2, 1.0), (0, 3, 0.5), (1, 3, 0.5), (2, 3, 0.5), (6, 7, 0.75)]:
        g[a, b] = g[b, a] = v
    for a in (6, 7):
        for b in (0, 1, 2, 3):
            g[a, b] = g[b, a] = 0.25
    for b in range(8):
        if b not in (4, 5):
            g[4, b] = g[b, 4] = -0.3
    np.fill_diagonal(g, 1.0)
    g[5, :] = g[:, 5] = 0.0
    return g, _gp(eps, 2, "cosine", "rational")


GRAM_FIXTURES = {
    "tie": tie_fixture, "eps": eps_fixture, "d1": d1_fixture, "d2": d2_fixture, "kclamp": kclamp_fixture,
    "l2_clamp": l2_clamp_fixture, "cosine_eps1": lambda: cosine_fixture(1.0), "cosine_eps09": lambda: cosine_fixture(0.9),
}


@functools.lru_cache(maxsize=None)
def expected_graph(name):
    gram, gp = GRAM_FIXTURES[name]()
    return oracle_np.feature_graph_from_gram(gram, oracle_np.resolve_params(gp))


# ------------------------------------------------------------------------------------------------ (a) items of the Gram stage
GRAM_DS = (1, 2, 127, 128, 129, 257)
GRAM_N = 80
GRAM_RANGES = ((0, 0), (5, 6), (3, 77), (0, GRAM_N))
GRAM_SPLIT = ((0, 3), (3, 77), (77, GRAM_N))
GRAM_BIG = (16421, 24)


@functools.lru_cache(maxsize=None)
def gram_items(n, d, storage):
    """Integers in [-3, 3]; storage "f64": three entries of the first and last column are 2^24 + 1, which fp32 cannot hold,
    so the space keeps its fp64 copy.  Every Gram entry stays an exact integer below 2^53 in any summation order."""
    X = np.random.default_rng(1000 * d + n).integers(-3, 4, (n, d)).astype(np.float64)
    if storage == "f64":
        for r, c in ((4, 0), (n // 2, d - 1), (n - 2, 0)):
            X[r, c] = 2.0 ** 24 + 1
    return X


def int_gram_of(X, r0, r1):
    Xi = X[r0:r1].astype(np.int64)
    G = Xi.T @ Xi
    assert (np.abs(Xi) ** 2).sum(0).max() < 2 ** 53 if r1 > r0 else True    # sum |x_a x_b| <= the largest column norm
    return G.astype(np.float64)


# ------------------------------------------------------------------------------------------------ (c) energy vectors
@functools.lru_cache(maxsize=None)
def path_fixture():
    """D = 12: two paths 0-1-...-5 and 6-7-...-11 of unit steps on a line (keys 1, the next ones 4), eps = 1, k = 2,
    sigma = 0.5: ten edges of one weight exp(-2)."""
    pos = np.array([0, 1, 2, 3, 4, 5, 100, 101, 102, 103, 104, 105])
    return _int_gram(pos[:, None]), _gp(1.0, 2, "l2", "gaussian", sigma=0.5)


def path_vectors(storage):
    """rows: 0 zero; 1 constant on each component; 2, 3 differ across one edge; 4, 5 across two edges by the same amount.
    -> (X, expected G per row).  storage "f64": scaled by 1 + 2^-30, which fp32 cannot hold."""
    X = np.zeros((6, 12))
    X[1, :6], X[1, 6:] = 3.0, -2.0
    X[2, 0] = 1.5
    X[3, :6], X[3, 6:11], X[3, 11] = 2.0, 7.0, 5.0
    X[4, 1] = 1.5
    X[5, :6], X[5, 6:] = -1.0, 4.0
    X[5, 8] = 4.75
    if storage == "f64":
        X = X * (1.0 + 2.0 ** -30)
    return X, np.array([0.0, 0.0, 1.0, 1.0, 0.5, 0.5])


RANGE_N, RANGE_D = 37, 40


@functools.lru_cache(maxsize=None)
def range_fixture():
    """37 random items of 40 features over the graph of 40 random integer columns (about a fifth of the pairs inside eps)."""
    rng = np.random.default_rng(37)
    gram = _int_gram(rng.integers(-3, 4, (RANGE_D, 6)))
    m = np.diagonal(gram)
    key = m[:, None] + m[None, :] - 2.0 * gram
    eps = float(np.sqrt(np.quantile(key[~np.eye(RANGE_D, dtype=bool)], 0.2)))
    return rng.standard_normal((RANGE_N, RANGE_D)), gram, _gp(eps, 4, "l2", "rational")


WIDE_SHAPES = ((50, 2401), (50, 3201), (1101, 4801))


@functools.lru_cache(maxsize=None)
def wide_fixture(n, d):
    """Items of d > 2400 features over a band graph: m_a = 2, g_ab = 1, 1.25 or 1.5 for |a - b| <= 2 (keys 2, 1.5, 1: three
    weights), eps^2 = 2, k = 4.  The Gram costs O(D) to write and its oracle a few D x D passes."""
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d))
    if d != 3201:
        X = X.astype(np.float32).astype(np.float64)          # fp32 storage; 3201 stays in fp64
    gram = np.zeros((d, d))
    a = np.arange(d)
    gram[a, a] = 2.0
    for off in (1, 2):
        lo = a[:-off]
        v = 1.0 + 0.25 * ((2 * lo + off) % 3)
        gram[lo, lo + off] = v
        gram[lo + off, lo] = v
    return X, gram, _gp(np.sqrt(2.0), 4, "l2", "gaussian", sigma=1.0)


def energy_launch(d, n, cus):
    """feat_energy's launch shape, restated from as_feat.hip: (waves per block, blocks, trips of the stride loop, rows of
    the last trip).  Two rows per wave; 16 d bytes of LDS per wave within 150 KiB; at most 8 blocks per CU, fewer when
    150 KiB / LDS per block is."""
    per_wave = 16 * d
    waves = max(1, min(4, (150 * 1024) // per_wave))
    lds = per_wave * waves
    per_cu = max(1, min(8, (150 * 1024) // lds))
    want = -(-n // (2 * waves))
    grid = max(1, min(want, cus * per_cu))
    per_trip = grid * waves * 2
    trips = -(-n // per_trip)
    return waves, grid, trips, n - (trips - 1) * per_trip


# ------------------------------------------------------------------------------------------------ (d) the ratio pass
SCALED_SHAPES = ((300, 24, 5), (401, 130, 8))
RATIO_SCALES = (240, -240)         # T beyond 1e+-140: feat_ratio_pass
CONTROL_SCALES = (200, -200)       # T inside: S2 / T^2


@functools.lru_cache(maxsize=None)
def scaled_base(n, d, k):
    """(X, gp) of the unscaled cosine / rational index; X does not round-trip through fp32 (fp64 storage)."""
    X = clustered(n, d, nclust=max(4, n // 64), seed=n + d)
    return X, dict(_gp(calibrate_feature_eps(X, k, "cosine"), k, "cosine", "rational"), topk=5)


@functools.lru_cache(maxsize=None)
def scaled_oracle(n, d, k, s):
    X, gp = scaled_base(n, d, k)
    return oracle_np.build_feature(np.ldexp(X, s), oracle_np.resolve_params(gp))


def edge_energy_sums(idx, X):
    """T of every row of X over the oracle index's edges."""
    diff = X[:, idx["ea"]] - X[:, idx["eb"]]
    return (idx["ew"][None, :] * diff * diff).sum(axis=1)
