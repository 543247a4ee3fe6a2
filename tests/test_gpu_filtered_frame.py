"""GPU: the call frame every filtered entry point shares ("the filtered call frame"), one table row
per entry point: the 8 subset / items forms, the 4 lists forms, range, fused, grouped and diversified search.  Two spaces are
built from the items of tests/golden/synth_64x24_l2.npz (n = 64, d = 24, topk = 4).  Through the C ABI every row is refused, one
wrong argument at a time, for a query of d + 1 features, a NaN tau (a sweep: in the last position), an id of n, an id of -1 (the
lists also: offsets that decrease) and a subset or groups handle of the other space; then with all of them wrong at once, which
pins the refusal that comes first.  Each refusal: the status, the message, every output buffer still holding its sentinel (but
for the out_len / out_ngroups zeroing and the range handle set to null, which come before the checks), and no counter of the
space moved.  Then one accepted call per row through the Python methods: repeated taus give identical rows, the batched forms
agree with the single forms the way the family's own suites define it (their helpers are used), calls and lambda_q steps are
counted once."""
import ctypes as C
import os

import numpy as np
import pytest

import grouped_ref
from conftest import clustered
from test_gpu_range import same_but_for_threshold_ties
from test_gpu_subset import same_as_single

pytestmark = pytest.mark.gpu

TAU, TAUS, IDS = 0.62, [0.5, 1.0, 0.5], [5, 5, 63, 0]
NG, PG, NDIV = 3, 2, 3
I64, F64, I32 = np.int64, np.float64, np.int32
SENTINEL = {I64: -7, F64: -7.5, I32: -7}


@pytest.fixture(scope="module")
def env():
    import pyarrowspace_amd as asp
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_64x24_l2.npz"))
    n, d = int(z["n"]), int(z["d"])
    X = clustered(n, d, nclust=int(z["nclust"]), seed=int(z["seed"]))
    gp = {"eps": float(z["eps"]), "k": int(z["k"]), "topk": int(z["topk"]), "p": 2.0, "sigma": None, "metric": str(z["metric"]),
          "kernel": str(z["kernel"])}
    e = type("Env", (), {})()
    e.asp, e.n, e.d, e.topk = asp, n, d, gp["topk"]
    e.a, e.gl = asp.ArrowSpaceBuilder.build(gp, X)
    e.other, e.other_gl = asp.ArrowSpaceBuilder.build(gp, X)
    e.Q = np.ascontiguousarray(z["Q"][:3])
    assert (z["lambda_q"][:3] != 0.0).all()
    e.labels = np.arange(n) // 7
    e.sub, e.their_sub = e.a.subset(IDS), e.other.subset(IDS)
    e.grp, e.their_grp = e.a.groups(e.labels), e.other.groups(e.labels)
    e.kk = min(e.topk, e.sub.size)
    return e


def p_i64(a):
    return C.cast(a.ctypes.data, C.POINTER(C.c_int64))


def p_f64(a):
    return C.cast(a.ctypes.data, C.POINTER(C.c_double))


class Args:
    """The inputs of one call: right ones, with those named in `wrong` replaced."""

    def __init__(self, e, batch, wrong=()):
        self.b = 3
        self.d = e.d + 1 if "d" in wrong else e.d
        Q = e.Q if self.d == e.d else np.ascontiguousarray(np.pad(e.Q, ((0, 0), (0, 1))))
        self.q = Q if batch else np.ascontiguousarray(Q[0])
        self.tau = float("nan") if "tau" in wrong else TAU
        self.taus = np.array(TAUS[:2] + [float("nan")] if "tau" in wrong else TAUS)
        self.nt = 3
        ids = list(IDS)
        if "id_hi" in wrong:
            ids[2] = e.n
        if "id_lo" in wrong:
            ids[3 if "id_hi" in wrong else 2] = -1   # (behind the id of n: the first wrong id is the one refused)
        self.ids = np.array(ids, dtype=I64)
        self.m = 4
        # the lists: every query its own copy of IDS; the wrong id sits in list 1
        lists = [list(IDS), ids, list(IDS)]
        self.list_ids = np.array(sum(lists, []), dtype=I64)
        self.offs = np.array([0, 4, 3, 12] if "offs" in wrong else [0, 4, 8, 12], dtype=I64)
        self.sub = (e.their_sub if "sub" in wrong else e.sub)._h
        self.grp = (e.their_grp if "groups" in wrong else e.grp)._h
        self.mins = np.full(3, -np.inf)


# One row per entry point: name -> (batch, the refusals beyond d and tau that apply, outputs, call).  An output is
# (dtype, entries, zeroed): zeroed outputs are set to 0 before the checks (a tuple: with these refusals only); "handle" is the
# range answer (set to null there).
def rows(e):
    kk, b, nt, k = e.kk, 3, 3, e.topk
    hits = lambda count: {"idx": (I64, count * kk, False), "sc": (F64, count * kk, False), "len": (I64, count, True)}
    lists_hits = lambda count: {"idx": (I64, count * k, False), "sc": (F64, count * k, False), "len": (I64, count, False)}
    one, per_q = {"lq": (F64, 1, False)}, {"lq": (F64, b, False), "st": (I32, b, False)}
    plain = {"lq": (F64, 1, ("d", "tau"))}   # the two plain single forms publish lambda_q = 0 with a refusal of the shared checks
    grouped = lambda count: {"label": (I64, count * NG, False), "count": (I64, count * NG, False), "idx": (I64, count * NG * PG, False),
                             "sc": (F64, count * NG * PG, False), "len": (I64, count, True)}
    diverse = lambda count: {"idx": (I64, count * NDIV, False), "sc": (F64, count * NDIV, False), "mg": (F64, count * NDIV, False),
                             "len": (I64, count, True)}
    L, sp, gr = e.asp._L, e.a._h, e.gl._h
    d_ = lambda a: a.ctypes.data
    return {
        "as_search_subset": (False, ("sub",), {**hits(1), **plain}, lambda A, O: L.as_search_subset(
            sp, gr, d_(A.q), A.d, A.tau, A.sub, d_(O["idx"]), d_(O["sc"]), p_i64(O["len"]), p_f64(O["lq"]))),
        "as_score_items": (False, ("id_hi", "id_lo"), {"out": (F64, 4, False), **plain}, lambda A, O: L.as_score_items(
            sp, gr, d_(A.q), A.d, A.tau, d_(A.ids), A.m, d_(O["out"]), p_f64(O["lq"]))),
        "as_search_subset_batch": (True, ("sub",), {**hits(b), **per_q}, lambda A, O: L.as_search_subset_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, A.sub, d_(O["idx"]), d_(O["sc"]), d_(O["len"]), d_(O["lq"]), d_(O["st"]))),
        "as_score_items_batch": (True, ("id_hi", "id_lo"), {"out": (F64, b * 4, False), **per_q}, lambda A, O: L.as_score_items_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, d_(A.ids), A.m, d_(O["out"]), d_(O["lq"]), d_(O["st"]))),
        "as_search_subset_taus": (False, ("sub",), {**hits(nt), **one}, lambda A, O: L.as_search_subset_taus(
            sp, gr, d_(A.q), A.d, d_(A.taus), A.nt, A.sub, d_(O["idx"]), d_(O["sc"]), d_(O["len"]), p_f64(O["lq"]))),
        "as_score_items_taus": (False, ("id_hi", "id_lo"), {"out": (F64, nt * 4, False), **one}, lambda A, O: L.as_score_items_taus(
            sp, gr, d_(A.q), A.d, d_(A.taus), A.nt, d_(A.ids), A.m, d_(O["out"]), p_f64(O["lq"]))),
        "as_search_subset_batch_taus": (True, ("sub",), {**hits(b * nt), **per_q}, lambda A, O: L.as_search_subset_batch_taus(
            sp, gr, d_(A.q), A.b, A.d, d_(A.taus), A.nt, A.sub, d_(O["idx"]), d_(O["sc"]), d_(O["len"]), d_(O["lq"]), d_(O["st"]))),
        "as_score_items_batch_taus": (True, ("id_hi", "id_lo"), {"out": (F64, b * nt * 4, False), **per_q},
                                      lambda A, O: L.as_score_items_batch_taus(
            sp, gr, d_(A.q), A.b, A.d, d_(A.taus), A.nt, d_(A.ids), A.m, d_(O["out"]), d_(O["lq"]), d_(O["st"]))),
        "as_score_lists_batch": (True, ("list_hi", "list_lo", "offs"), {"out": (F64, 12, False), **per_q}, lambda A, O: L.as_score_lists_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, d_(A.list_ids), d_(A.offs), d_(O["out"]), d_(O["lq"]), d_(O["st"]))),
        "as_search_lists_batch": (True, ("list_hi", "list_lo", "offs"), {**lists_hits(b), **per_q}, lambda A, O: L.as_search_lists_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, d_(A.list_ids), d_(A.offs), d_(O["idx"]), d_(O["sc"]), d_(O["len"]), d_(O["lq"]), d_(O["st"]))),
        "as_score_lists_batch_taus": (True, ("list_hi", "list_lo", "offs"), {"out": (F64, nt * 12, False), **per_q},
                                      lambda A, O: L.as_score_lists_batch_taus(
            sp, gr, d_(A.q), A.b, A.d, d_(A.taus), A.nt, d_(A.list_ids), d_(A.offs), d_(O["out"]), d_(O["lq"]), d_(O["st"]))),
        "as_search_lists_batch_taus": (True, ("list_hi", "list_lo", "offs"), {**lists_hits(b * nt), **per_q},
                                       lambda A, O: L.as_search_lists_batch_taus(
            sp, gr, d_(A.q), A.b, A.d, d_(A.taus), A.nt, d_(A.list_ids), d_(A.offs), d_(O["idx"]), d_(O["sc"]), d_(O["len"]), d_(O["lq"]),
            d_(O["st"]))),
        "as_search_range": (False, ("sub",), {"handle": None, **one}, lambda A, O: L.as_search_range(
            sp, gr, d_(A.q), A.d, A.tau, -np.inf, A.sub, 0, C.byref(O["handle"]), p_f64(O["lq"]))),
        "as_search_range_batch": (True, ("sub",), {"handle": None, **per_q}, lambda A, O: L.as_search_range_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, d_(A.mins), A.sub, 0, C.byref(O["handle"]), d_(O["lq"]), d_(O["st"]))),
        "as_search_fused": (True, ("sub",), {**hits(1), **per_q}, lambda A, O: L.as_search_fused(
            sp, gr, d_(A.q), A.b, A.d, A.tau, None, 0, 0, A.sub, d_(O["idx"]), d_(O["sc"]), p_i64(O["len"]), d_(O["lq"]), d_(O["st"]))),
        "as_score_fused": (True, ("id_hi", "id_lo"), {"out": (F64, 4, False), **per_q}, lambda A, O: L.as_score_fused(
            sp, gr, d_(A.q), A.b, A.d, A.tau, None, 0, 0, d_(A.ids), A.m, d_(O["out"]), d_(O["lq"]), d_(O["st"]))),
        "as_search_grouped": (False, ("sub", "groups"), {**grouped(1), **one}, lambda A, O: L.as_search_grouped(
            sp, gr, d_(A.q), A.d, A.tau, A.grp, NG, PG, A.sub, d_(O["label"]), d_(O["count"]), d_(O["idx"]), d_(O["sc"]), p_i64(O["len"]),
            p_f64(O["lq"]))),
        "as_search_grouped_batch": (True, ("sub", "groups"), {**grouped(b), **per_q}, lambda A, O: L.as_search_grouped_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, A.grp, NG, PG, A.sub, d_(O["label"]), d_(O["count"]), d_(O["idx"]), d_(O["sc"]), d_(O["len"]),
            d_(O["lq"]), d_(O["st"]))),
        "as_search_diverse": (False, ("sub",), {**diverse(1), **one}, lambda A, O: L.as_search_diverse(
            sp, gr, d_(A.q), A.d, A.tau, NDIV, 0.5, A.sub, d_(O["idx"]), d_(O["sc"]), d_(O["mg"]), p_i64(O["len"]), p_f64(O["lq"]))),
        "as_search_diverse_batch": (True, ("sub",), {**diverse(b), **per_q}, lambda A, O: L.as_search_diverse_batch(
            sp, gr, d_(A.q), A.b, A.d, A.tau, NDIV, 0.5, A.sub, d_(O["idx"]), d_(O["sc"]), d_(O["mg"]), d_(O["len"]), d_(O["lq"]), d_(O["st"]))),
    }


ROWS = ("as_search_subset", "as_score_items", "as_search_subset_batch", "as_score_items_batch", "as_search_subset_taus",
        "as_score_items_taus", "as_search_subset_batch_taus", "as_score_items_batch_taus", "as_score_lists_batch", "as_search_lists_batch",
        "as_score_lists_batch_taus", "as_search_lists_batch_taus", "as_search_range", "as_search_range_batch", "as_search_fused",
        "as_score_fused", "as_search_grouped", "as_search_grouped_batch", "as_search_diverse", "as_search_diverse_batch")

COUNTERS = (("as_search_counters", 8), ("as_sweep_counters", 3), ("as_batch_sweep_counters", 4), ("as_subset_sweep_counters", 4),
            ("as_lists_counters", 5), ("as_lists_sweep_counters", 6), ("as_range_counters", 6), ("as_fused_counters", 4),
            ("as_grouped_counters", 7), ("as_diverse_counters", 5))


def all_counters(e):
    """Every counter of the space (the lists' include host nanoseconds: a refused call adds none)."""
    got = {}
    for name, count in COUNTERS:
        out = (C.c_int64 * count)()
        assert getattr(e.asp._L, name)(e.a._h, out, count) == 0
        got[name] = list(out)
    return got


def refusals(e, who, wrongs):
    """(the wrong arguments, the message) of every refusal of a row, one wrong argument at a time, in the frame's order; last:
    all of them at once with the message of the refusal that comes first."""
    n, d = e.n, e.d
    msg = {"d": f"query length {d + 1} must match nfeatures {d}", "tau": f"{who}: tau must be finite",
           "id_hi": f"{who}: id {n} is outside [0, {n})", "id_lo": f"{who}: id -1 is outside [0, {n})",
           "list_hi": f"{who}: id {n} of list 1 is outside [0, {n})", "list_lo": f"{who}: id -1 of list 1 is outside [0, {n})",
           "offs": f"{who}: offsets must not decrease (offsets[2] = 3 after 4)", "sub": f"{who}: the subset was made for another space",
           "groups": f"{who}: the groups were made for another space"}
    arg = {"list_hi": "id_hi", "list_lo": "id_lo"}
    each = [((arg.get(w, w),), msg[w]) for w in ("d", "tau") + wrongs]
    # what is looked at first today: the handles (the groups before the subset) and the ids of the items forms come before
    # d and tau, the lists' offsets and ids after them
    first = "groups" if "groups" in wrongs else "sub" if "sub" in wrongs else "id_hi" if "id_hi" in wrongs else "d"
    everything = tuple(dict.fromkeys(arg.get(w, w) for w in ("d", "tau") + wrongs))
    return each + [(everything, msg[first])]


@pytest.mark.parametrize("who", ROWS)
def test_refusals_leave_outputs_and_counters_alone(env, who):
    e = env
    batch, wrongs, outs, call = rows(e)[who]
    for wrong, message in refusals(e, who, wrongs):
        A = Args(e, batch, wrong)
        O = {name: C.c_void_p(1234) if spec is None else np.full(max(spec[1], 1), SENTINEL[spec[0]], dtype=spec[0])
             for name, spec in outs.items()}
        before = all_counters(e)
        status = call(A, O)
        text = e.asp._lib.last_error()
        assert status == e.asp._lib.AS_EINVAL, (wrong, status, text)
        assert message in text, (wrong, text)
        for name, spec in outs.items():
            if spec is None:
                assert O[name].value is None, (wrong, name)
            elif spec[2] is True or (spec[2] and wrong[0] in spec[2] and len(wrong) == 1):
                assert (O[name][:spec[1]] == 0).all(), (wrong, name, O[name])
            else:
                assert (O[name] == SENTINEL[spec[0]]).all(), (wrong, name, O[name])
        assert all_counters(e) == before, wrong


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def same_lists(a, b):
    assert [i for i, _ in a] == [i for i, _ in b] and bits([v for _, v in a]) == bits([v for _, v in b]), (a, b)


def moved(e, getter, keys=("calls", "lambda_steps")):
    c = getattr(e.a, getter)()
    return [c[k] for k in keys] if isinstance(c, dict) else [c[0], c[3]]   # (fused_counters is a list: calls, ..., lambda_q steps)


@pytest.fixture(scope="module")
def singles(env):
    """The single forms' answers the batched rows are held against, computed once."""
    e = env
    s = type("Singles", (), {})()
    s.hits = {(i, tau): e.a.search_subset(e.Q[i], e.gl, tau, e.sub) for i in range(3) for tau in set(TAUS) | {TAU}}
    s.scores = {(i, tau): e.a.score_items(e.Q[i], e.gl, tau, IDS) for i in range(3) for tau in set(TAUS) | {TAU}}
    return s


def test_accepted_subset_and_items_forms(env, singles):
    e, a, gl, Q = env, env.a, env.gl, env.Q
    c0 = moved(e, "subset_sweep_counters")
    assert len(singles.hits[0, TAU]) == e.kk
    assert bits(singles.scores[0, TAU][0]) == bits(singles.scores[0, TAU][1])   # ids[0] == ids[1]
    batched = a.search_batch_subset(Q, gl, TAU, e.sub)
    rows_b = a.score_items_batch(Q, gl, TAU, IDS)
    for i in range(3):
        same_as_single(batched[i], singles.hits[i, TAU])
        np.testing.assert_allclose(rows_b[i], singles.scores[i, TAU], rtol=1e-12, atol=0.0)
    assert moved(e, "subset_sweep_counters") == c0   # (the plain forms are no sweeps)
    swept, rows_t = a.search_subset_taus(Q[0], gl, TAUS, e.sub), a.score_items_taus(Q[0], gl, TAUS, IDS)
    same_lists(swept[0], swept[2])
    assert bits(rows_t[0]) == bits(rows_t[2])
    for j, tau in enumerate(TAUS):
        same_as_single(swept[j], singles.hits[0, tau])
        np.testing.assert_allclose(rows_t[j], singles.scores[0, tau], rtol=1e-12, atol=0.0)
    swept_b, rows_bt = a.search_batch_subset_taus(Q, gl, TAUS, e.sub), a.score_items_batch_taus(Q, gl, TAUS, IDS)
    for i in range(3):
        same_lists(swept_b[i][0], swept_b[i][2])
        assert bits(rows_bt[i, 0]) == bits(rows_bt[i, 2])
        for j, tau in enumerate(TAUS):
            same_as_single(swept_b[i][j], singles.hits[i, tau])
            np.testing.assert_allclose(rows_bt[i, j], singles.scores[i, tau], rtol=1e-12, atol=0.0)
    assert moved(e, "subset_sweep_counters") == [c0[0] + 4, c0[1] + 4]


def test_accepted_lists_forms(env, singles):
    e, a, gl, Q = env, env.a, env.gl, env.Q
    lists = [IDS, IDS, IDS]
    c0, s0 = moved(e, "lists_counters"), moved(e, "lists_sweep_counters")
    got, rows_l = a.search_batch_lists(Q, gl, TAU, lists), a.score_lists_batch(Q, gl, TAU, lists)
    for i in range(3):
        same_as_single(got[i], singles.hits[i, TAU])
        np.testing.assert_allclose(rows_l[i], singles.scores[i, TAU], rtol=1e-12, atol=0.0)
    assert moved(e, "lists_counters") == [c0[0] + 2, c0[1] + 2] and moved(e, "lists_sweep_counters") == s0
    swept, rows_t = a.search_batch_lists_taus(Q, gl, TAUS, lists), a.score_lists_batch_taus(Q, gl, TAUS, lists)
    for i in range(3):
        same_lists(swept[i][0], swept[i][2])
        assert bits(rows_t[i][0]) == bits(rows_t[i][2])
        for j, tau in enumerate(TAUS):
            same_as_single(swept[i][j], singles.hits[i, tau])
            np.testing.assert_allclose(rows_t[i][j], singles.scores[i, tau], rtol=1e-12, atol=0.0)
    assert moved(e, "lists_counters") == [c0[0] + 2, c0[1] + 2] and moved(e, "lists_sweep_counters") == [s0[0] + 2, s0[1] + 2]


def test_accepted_range_fused_grouped_and_diverse_forms(env, singles):
    e, a, gl, Q = env, env.a, env.gl, env.Q
    thr = float(np.sort(singles.scores[0, TAU])[1])
    c0 = moved(e, "range_counters")
    single = [a.search_range(Q[i], gl, TAU, thr, e.sub) for i in range(3)]
    assert bits([v for _, v in single[0]]) == bits([v for v in sorted(set(singles.scores[0, TAU].tolist()), reverse=True) if v >= thr])
    batched = a.search_range_batch(Q, gl, TAU, thr, e.sub)
    for i in range(3):
        same_but_for_threshold_ties(batched[i], single[i], thr)
    assert moved(e, "range_counters") == [c0[0] + 4, c0[1] + 4]
    # fused: the selection and the score form give one accumulator's bits
    c0 = moved(e, "fused_counters")
    hits = a.search_fused(Q, gl, TAU, subset=e.sub)
    F = a.score_fused(Q, gl, TAU, IDS)
    assert len(hits) == e.kk and bits(F[0]) == bits(F[1])
    assert bits([v for _, v in hits]) == bits([F[IDS.index(i)] for i, _ in hits])
    assert moved(e, "fused_counters") == [c0[0] + 2, c0[1] + 2]
    # grouped: the numpy reference over the bits of score_items (single) / score_items_batch (batched), as in test_gpu_grouped.py
    ids = np.sort(np.unique(IDS))
    c0 = moved(e, "grouped_counters")
    flat = lambda r: [(int(l), [(int(i), bits(v)) for i, v in mem]) for l, mem in r]
    for i in range(3):
        want = grouped_ref.grouped(ids, e.labels[ids], a.score_items(Q[i], gl, TAU, ids), NG, PG)
        assert flat(a.search_grouped(Q[i], gl, TAU, e.grp, NG, PG, subset=e.sub)) == flat(want)
    got = a.search_batch_grouped(Q, gl, TAU, e.grp, NG, PG, subset=e.sub)
    S = a.score_items_batch(Q, gl, TAU, ids)
    for i in range(3):
        assert flat(got[i]) == flat(grouped_ref.grouped(ids, e.labels[ids], S[i], NG, PG))
    assert moved(e, "grouped_counters") == [c0[0] + 4, c0[1] + 4]
    # diversified, diversity 0: the head of the pool as it is -- search_subset's list, search_batch_subset's for the batched form
    c0 = moved(e, "diverse_counters", ("calls", "pool_steps"))
    for i in range(3):
        same_lists(a.search_diverse(Q[i], gl, TAU, NDIV, 0.0, subset=e.sub), singles.hits[i, TAU][:NDIV])
    got, pools = a.search_batch_diverse(Q, gl, TAU, NDIV, 0.0, subset=e.sub), a.search_batch_subset(Q, gl, TAU, e.sub)
    for i in range(3):
        same_lists(got[i], pools[i][:NDIV])
        same_as_single(got[i], singles.hits[i, TAU][:NDIV])
    assert moved(e, "diverse_counters", ("calls", "pool_steps")) == [c0[0] + 4, c0[1] + 4]
