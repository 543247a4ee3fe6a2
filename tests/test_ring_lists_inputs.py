"""CPU: the hand-built inputs of tests/test_gpu_ring_lists.py are what that file takes them for, and the numpy model
(oracle_np.ring_fold / ring_merge / ring_thresholds) agrees on them with an independent restatement: sorted() per row and
Fraction arithmetic for every bound, so no fp64 rounding is shared with the model.  Every "edge +- 1 ulp" input lies on the
side its name says, the exact coefficient's products are exact, the roundings the kernels are tested for really occur
(a bound whose rounding to nearest differs from its rounding down / up), and the soundness inputs flag between 20 % and
80 % of their rows under both metrics and both routes."""
import math
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_ring_lists as rl
from oracle import oracle_np

INF = float("inf")


def _frac(x):
    return Fraction(float(x))


def _err(metric, n_i, nmax, coef=rl.COEF):
    """e as a rational."""
    return _frac(coef) * (_frac(n_i) + _frac(nmax)) if metric == "l2" else _frac(coef)


def _bound_minus(t32, e):
    """rd32(t32 - e) without fp64: the largest fp32 not above the rational."""
    t = float(t32)
    if math.isinf(t) or math.isnan(t):
        return np.float32(t)
    return rl.f32_floor(_frac(t) - e)


def _entries(sl, r):
    c = int(sl[4][r]) & 0xFFFF
    return [(float(sl[0][r, t]), int(sl[3][r, t]), float(sl[1][r, t]), float(sl[2][r, t])) for t in range(c)]


def dumb_fold(run, blk, M, metric, n_rows, nmax_b, mode, flag):
    """-> per row None (does not take part) or (entries, count word, bound)."""
    out = []
    for r in range(len(run[4])):
        if mode != 0 and not flag[r]:
            out.append(None)
            continue
        ents = ([] if mode == 2 else _entries(run, r)) + _entries(blk, r)
        assert len({(e[0], e[1]) for e in ents}) == len(ents)             # equal (key, id) pairs are never fed
        ents = sorted(ents, key=lambda e: (e[0], e[1]))[:M]
        d_run = mode != 2 and bool(int(run[4][r]) >> 30 & 1)
        d_blk = bool(int(blk[4][r]) >> 30 & 1)
        bounds = [np.float32(INF)]
        if d_run:
            bounds.append(run[5][r])
        if d_blk:
            bounds.append(_bound_minus(blk[5][r], _err(metric, n_rows[r], nmax_b)))
        out.append((ents, len(ents) | (int(d_run or d_blk) << 30), min(bounds)))
    return out


def check_fold(model, dumb, run, M):
    for r, d in enumerate(dumb):
        if d is None:
            for j in range(6):
                assert np.array_equal(rl._bits(model[j][r]), rl._bits(run[j][r]))
            continue
        ents, word, bound = d
        assert int(model[4][r]) == word
        assert rl._bits(model[5][r]).item() == rl._bits(bound).item(), (r, model[5][r], bound)
        assert _entries(model, r) == ents


def dumb_merge(case, k, metric):
    slices, nmax = case["slices"], case["block_nmax"]
    eps = case["eps"]
    ek = eps * eps if metric == "l2" else eps
    out = []
    for r in range(len(slices[0][4])):
        ents = [e for s in slices for e in _entries(s, r)]
        ok = sorted([e for e in ents if e[0] <= ek], key=lambda e: (e[0], e[1]))
        B = ok[k - 1][0] if len(ok) >= k else ek
        flag = 0
        for b, s in enumerate(slices):
            if not int(s[4][r]) >> 30 & 1:
                continue
            t = float(s[5][r])
            if math.isnan(t) or t == -INF:
                flag = 1
            elif t != INF and not (_frac(t) - (0 if nmax is None else _err(metric, case["n_rows"][r], nmax[b])) > _frac(B)):
                flag = 1
        out.append((ok[:k], B, flag))
    return out


# ------------------------------------------------------------------------------------------------ the space
def test_space_norms_are_dyadic_and_differ_from_row_to_row():
    X, n = rl.space_items()
    assert X.shape == (rl.SPACE_N, rl.D) and set(np.unique(np.abs(X))) <= {0.0, 0.5, 1.0, 2.0}
    assert np.array_equal(n, np.einsum("ij,ij->i", X, X)) and n[5] == 0.0 and (np.delete(n, 5) > 0).all()
    for s in (1, 2, 3, 4):
        assert (n[s:] != n[:-s]).all()               # a wrong row offset of up to 4 reads another norm at EVERY row
    assert (n * 4 == np.round(n * 4)).all() and n.max() <= 32.0
    assert max(rl.ROW_SIZES) + 3 < rl.SPACE_N


def test_exact_coefficient_products_are_exact():
    """coef * (n_i + nmax) for every norm and block maximum the exact-coefficient tests use, the soundness inputs included."""
    assert rl.COEF == oracle_np.ring_coef_i8(0.0, 2.0 ** -6) and _frac(rl.COEF) == Fraction(1, 2 ** 12) + Fraction(12, 2 ** 24)
    n = rl.space_items()[1]
    own = float(n.max())
    for nmax in (0.25, 2.75, 9.5, 33.0, own, own + 7.5):
        for ni in np.unique(n):
            assert _frac(ni) + _frac(nmax) == _frac(ni + nmax)
            assert _frac(rl.COEF) * _frac(ni + nmax) == _frac(rl.COEF * (ni + nmax))
    for metric in ("l2", "cosine"):
        c = rl.soundness_case(metric)
        assert np.array_equal(c["n64"], np.einsum("ij,ij->i", c["X"], c["X"])) and (c["n64"] * 64 == np.round(c["n64"] * 64)).all()
        for nmax in c["block_nmax"]:
            for ni in np.unique(c["n64"]):
                assert _frac(rl.COEF) * (_frac(ni) + _frac(nmax)) == _frac(rl.COEF * (ni + nmax))
    # the default coefficient's product is NOT exact (the test under it compares against a Fraction and allows a step)
    coef = oracle_np.ring_coef_default(rl.DP)
    assert coef == (6 * 32 + 32) * 2.0 ** -24 + 3.03 * 2.0 ** -16
    assert any(_frac(coef) * _frac(ni + 9.5) != _frac(coef * (ni + 9.5)) for ni in np.unique(n))


# ------------------------------------------------------------------------------------------------ fold
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k", rl.WIDTHS)
def test_fold_model_agrees_with_the_restatement(M, k, metric):
    seen, rne_differs = set(), 0
    for rows, row_begin, mode in rl.FOLD_CONFIGS:
        c = rl.fold_case(M, metric, rows, row_begin, mode)
        run, blk = c["run"], c["blk"]
        model = rl.fold_expected(c, M, metric, mode)
        check_fold(model, dumb_fold(run, blk, M, metric, c["n_rows"], c["nmax_b"], mode, c["flag"]), run, M)
        assert (run[4] & 0x3FFF0000 == 0).all() and (blk[4] & 0x3FFF0000 == 0).all()        # bits 16-29 clear, as the producers write
        assert ((run[4] & 0xFFFF) <= M).all() and ((blk[4] & 0xFFFF) <= M).all()            # the kernel's LDS holds 2 M entries
        for sl in (run, blk):
            for r in range(rows):
                e = _entries(sl, r)
                assert e == sorted(e, key=lambda x: (x[0], x[1]))
        if mode:
            assert 0 < int((c["flag"] != 0).sum()) < rows or rows == 1
        pats = rl.fold_patterns(M)
        for r, kind in enumerate(c["kinds"]):
            cr, cb = int(run[4][r]) & 0xFFFF, int(blk[4][r]) & 0xFFFF
            seen.add(((cr, cb), (int(run[4][r]) >> 30, int(blk[4][r]) >> 30), kind, mode if rows == 1027 else None))
            bt, rt = float(blk[5][r]), run[5][r]
            if kind in ("run_below", "run_above", "run_equal"):
                exact = _frac(bt) - _err(metric, c["n_rows"][r], c["nmax_b"])
                nb = rl.f32_floor(exact)
                assert _frac(nb) <= exact < _frac(np.nextafter(nb, rl.F32_INF))
                assert {"run_below": np.nextafter(rt, rl.F32_INF) == nb and _frac(rt) < _frac(nb),
                        "run_above": np.nextafter(rt, -rl.F32_INF) == nb and _frac(rt) > _frac(nb), "run_equal": rt == nb}[kind]
                rne_differs += int(np.float32(bt - rl.COEF * ((c["n_rows"][r] + c["nmax_b"]) if metric == "l2" else 1.0)) != nb)
            else:
                assert {"blk_pinf": bt == INF, "blk_ninf": bt == -INF, "run_pinf": rt == rl.F32_INF}[kind]
        # ties across the two lists, decided by id
        both = [r for r in range(rows) if {e[0] for e in _entries(run, r)} & {e[0] for e in _entries(blk, r)}]
        assert both or rows < 100
    # at 1027 rows every pattern occurs in every mode (C = M - 1, M, M + 1, 0 + 0, M + M, a block slice 0 | 1 << 30, ...)
    for mode in (0, 1, 2):
        assert {(cc, bb, kind, mode) for cc, bb, kind in rl.fold_patterns(M)} <= seen
    assert {sum(cc) for cc, _, _ in rl.fold_patterns(M)} >= {0, M - 1, M, M + 1, 2 * M}
    assert rne_differs > 50                      # a plain cast in place of the rounding down would show


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k", rl.WIDTHS)
def test_chain_model_agrees_with_the_restatement(M, k, metric):
    blocks, nmax, modes, flag, n_rows = rl.chain_case(M, metric)
    want = rl.chain_expected(M, metric)
    run = rl.empty_slice(len(flag), M)
    for step, (sl, nm, mode) in enumerate(zip(blocks, nmax, modes)):
        check_fold(want[step], dumb_fold(run, sl, M, metric, n_rows, nm, mode, flag), run, M)
        run = want[step]
    assert modes == [0, 0, 0, 0, 0, 2, 1] and 0 < flag.sum() < len(flag)
    full = (want[4][4] & 0xFFFF) == M
    assert full.any() and not full.all()
    assert ((want[5][4] & 0xFFFF)[flag != 0] <= (blocks[5][4] & 0xFFFF)[flag != 0]).all()          # mode 2 discarded the running lists
    ids = [set(b[3][b[3] != rl.POISON_ID].tolist()) for b in blocks]
    assert all(not (ids[i] & ids[j]) for i in range(7) for j in range(i))


def test_default_coefficient_case_leaves_the_block_bound_alone_to_decide():
    for metric in ("l2", "cosine"):
        c = rl.default_coef_case(metric)
        assert (c["run"][4] == 0).all() and (c["blk"][4] == 1 << 30).all() and np.isfinite(c["blk"][5]).all()
        assert c["row_begin"] + len(c["flag"]) <= rl.SPACE_N


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("M,k,nblocks,row_begin", rl.MERGE_CONFIGS)
def test_merge_model_agrees_with_the_restatement_and_the_kinds(M, k, nblocks, row_begin, metric):
    c = rl.merge_case(M, k, metric, nblocks, row_begin)
    model = rl.merge_expected(c, M, k, metric)
    eps = c["eps"]
    ek = eps * eps if metric == "l2" else eps
    slices = c["slices"]
    assert len(slices) == max(nblocks, 1) and (c["block_nmax"] is None) == (nblocks == 0)
    npass_kinds, at_eps, above_eps, nan_keys, ties = set(), 0, 0, 0, 0
    for r, (ents, B, flag) in enumerate(dumb_merge(c, k, metric)):
        m = len(ents)
        assert model["cnt"][r] == m and model["flag"][r] == flag == rl.EXPECT_FLAG[c["kinds"][r]], (r, c["kinds"][r])
        assert model["idx"][r, :m].tolist() == [e[1] for e in ents] and (model["idx"][r, m:] == -1).all()
        assert model["key"][r, :m].tolist() == [e[0] for e in ents]
        assert model["dist"][r, :m].tolist() == [e[2] for e in ents] and model["gy"][r, :m].tolist() == [e[3] for e in ents]
        assert (model["band"][r] == B) if flag else math.isnan(model["band"][r])
        every = [e for s in slices for e in _entries(s, r)]
        assert len({e[1] for e in every}) == len(every)
        for s in slices:
            assert int(s[4][r]) & 0x3FFF0000 == 0 and (int(s[4][r]) & 0xFFFF) <= M
            e = [x for x in _entries(s, r) if not math.isnan(x[0])]
            assert e == sorted(e, key=lambda x: (x[0], x[1]))
        npass = sum(1 for e in every if e[0] <= ek)
        npass_kinds.add("lt" if npass < k else "eq" if npass == k else "gt")
        at_eps += any(e[0] == ek for e in every)
        above_eps += any(e[0] == np.nextafter(ek, INF) for e in every)
        nan_keys += any(math.isnan(e[0]) for e in every)
        passing = sorted([e for e in every if e[0] <= ek], key=lambda x: (x[0], x[1]))
        ties += len(passing) > k and passing[k - 1][0] == passing[k][0]
        # the edges, in rationals: bound - e against B
        kind, star = c["kinds"][r], c["stars"][r]
        t = slices[star][5][r]
        e_star = 0 if nblocks == 0 else _err(metric, c["n_rows"][r], c["block_nmax"][star])
        if kind.startswith("edge"):
            assert int(slices[star][4][r]) >> 30 & 1 and npass >= k
            on = {"edge_equal": t, "edge_above": np.nextafter(t, -rl.F32_INF), "edge_below": np.nextafter(t, rl.F32_INF)}[kind]
            assert _frac(on) - e_star == _frac(B)
            margin = _frac(t) - e_star - _frac(B)
            assert {"edge_equal": margin == 0, "edge_above": margin > 0, "edge_below": margin < 0}[kind]
        if kind.startswith("zero_entry"):
            assert int(slices[star][4][r]) == 1 << 30                     # no entry, the dropped bit
        if kind == "none":
            assert not any(int(s[4][r]) >> 30 & 1 for s in slices)
            assert all(math.isnan(float(s[5][r])) or float(s[5][r]) == -INF for s in slices)
        if kind in ("far_below", "neg_inf", "nan", "edge_equal", "edge_below", "zero_entry_unproven") and len(slices) > 1:
            others = [b for b in range(len(slices)) if b != star and int(slices[b][4][r]) >> 30 & 1]
            assert all(float(slices[b][5][r]) - 0.25 > B for b in others)          # one unproven slice among the rest
    assert model["nflagged"] == int(model["flag"].sum()) and 0 < model["nflagged"] < rl.MERGE_ROWS
    assert set(c["kinds"]) >= set(rl.PROOF_KINDS) - ({"edge_equal", "edge_above", "edge_below"} if nblocks < 2 and k > 100 else set())
    assert {"edge_equal", "edge_above", "edge_below"} <= set(c["kinds"])
    assert npass_kinds == {"lt", "eq", "gt"} or (nblocks < 2 and npass_kinds >= {"lt", "gt"})
    assert above_eps > 5 and nan_keys > 5 and (at_eps > 5 or (nblocks < 2 and k > 100)) and ties > 5


def test_merge_configs_cover_what_the_issue_lists():
    at128 = {nb for M, k, nb, _ in rl.MERGE_CONFIGS if M == 128}
    assert at128 == {0, 1, 2, 5, 18} and {M for M, _, _, _ in rl.MERGE_CONFIGS} == {32, 64, 128}
    assert 4 * 16 * 18 * 128 <= 150 * 1024 < 4 * 16 * 19 * 128           # the host's LDS check admits 18 blocks, not 19
    assert rl.MERGE_ROWS % 4 and rl.MERGE_ROWS > 2 * len(rl.MERGE_KINDS)


# ------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("M,k", rl.WIDTHS)
def test_threshold_inputs_and_model(M, k):
    own = float(rl.space_items()[1].max())
    ru_differs = 0
    for metric in ("l2", "cosine"):
        for rows in rl.THRESHOLD_ROWS:
            for row_begin in (0, 3):
                key, cnt, n_rows = rl.thresholds_case(M, rows, row_begin)
                assert rows < 3 or set((cnt & 0xFFFF).tolist()) == {M - 1, M} and (cnt >> 30).any()
                for nmax_all in (0.25, own + 7.5):
                    nm = max(nmax_all, own)
                    thr = oracle_np.ring_thresholds(key, cnt, M, rl._metric(metric), rl.COEF, n_rows, nm)
                    for r in range(rows):
                        if (int(cnt[r]) & 0xFFFF) < M:
                            assert thr[r] == INF and math.isnan(key[r, M - 1])
                            continue
                        exact = _frac(key[r, M - 1]) + _err(metric, n_rows[r], nm)          # the bound that must hold
                        assert exact * Fraction(10000009, 10000000) < _frac(thr[r]) < exact * Fraction(1000002, 1000000)
                        x = (key[r, M - 1] + rl.COEF * ((n_rows[r] + nm) if metric == "l2" else 1.0)) * 1.000001
                        assert _frac(np.nextafter(thr[r], -rl.F32_INF)) < _frac(x) <= _frac(thr[r])
                        ru_differs += int(np.float32(x) != thr[r])
    assert ru_differs > 50                       # a plain cast in place of the rounding up would show


# ------------------------------------------------------------------------------------------------ soundness
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_soundness_inputs_flag_a_fifth_to_four_fifths_of_the_rows(metric):
    c = rl.soundness_case(metric)
    run, folded, unfolded = rl.soundness_expected(metric)
    b_idx, b_key, b_cnt = c["brute"]
    assert [len(s[4]) for s in c["slices"]] == [rl.SOUND_N] * 5 and rl.SOUND_CUTS[-1] == rl.SOUND_N
    for res in (folded, unfolded):
        share = res["nflagged"] / rl.SOUND_N
        assert 0.2 <= share <= 0.8, share
        ok = res["flag"] == 0
        # truthful slices: the model's unflagged rows ARE the brute-force lists
        assert np.array_equal(res["cnt"][ok], b_cnt[ok]) and np.array_equal(res["idx"][ok], b_idx[ok])
    assert (folded["flag"] >= unfolded["flag"]).all()
    # the restatement agrees on the merge of the five slices
    case = dict(slices=c["slices"], block_nmax=c["block_nmax"], eps=c["eps"], n_rows=c["n64"])
    for r, (ents, B, flag) in enumerate(dumb_merge(case, rl.SOUND_K, metric)):
        assert unfolded["flag"][r] == flag and unfolded["idx"][r, : len(ents)].tolist() == [e[1] for e in ents]
    # every slice is truthful: what it dropped is not below its bound, and the cut widths all occur
    widths = set()
    for b, s in enumerate(c["slices"]):
        size = rl.SOUND_CUTS[b + 1] - rl.SOUND_CUTS[b]
        for r in range(rl.SOUND_N):
            kept = int(s[4][r]) & 0xFFFF
            avail = size - (rl.SOUND_CUTS[b] <= r < rl.SOUND_CUTS[b + 1])
            assert bool(int(s[4][r]) >> 30) == (kept < avail)
            if kept < avail:
                widths.add(kept)
                assert s[5][r] >= oracle_np.rd32(float(s[0][r, kept - 1]))       # (what was dropped is not below what was kept)
            else:
                assert s[5][r] == rl.F32_INF
    assert widths == {8, 16, 32}
