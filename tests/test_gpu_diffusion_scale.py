"""GPU: the diffusion family at the sizes where its reductions take a second trip, and the modes and
budgets that the three modules of the family leave alone.  The shapes of tests/test_gpu_diffuse.py have 257 and 1 000 items and the
eigensolver's primitives go up to 2 053 rows, so a strand of either halving tree meets one pair per level, the Gram has one
partial in the solver's runs, the uncapped grid never wraps and the byte budgets never decide a chunk's width.  Here:
  - the Gram's tree (16 strands per entry) and the column norms' (256 strands) at 33 797 rows: 34 and 529 segments, a level of more
    than 2 x 16 and 2 x 256 pairs in trees padded to 64 and 1 024; at 32 768 rows, the last size without a second trip and
    without padding; and at 60 421 rows (60 and 945 segments), where pairs of the second trip add partials that exist -- at
    33 797 they all add padding, and a strand that skipped one of them would return the same bits;
  - shapes L and M of diffuse_ref.SCALE_SHAPES (131 137 and 230 337 items): the solve's tree (1 024 threads per column) over
    2 050 segments, the fewest that give it a second trip, and over 3 600, where 528 pairs of that trip add partials that exist;
    for a 16-wide chunk and for one column, and the recurrence over more rows than one trip of the uncapped grid;
  - eigsh on shape C (2 053 items, three Gram partials, the value 1 with multiplicity 19 ahead of a gap of 1.2e-3);
  - "diffuse_mib" and "diffuse_solve_mib" choosing 64, 16 or 1 columns on shape C;
  - "diffuse_timing": the timed calls of eigsh and of the solve return the untimed bits and fill their timers;
  - two host threads on eigsh, the solve and the recurrence of one space.
Every expected value comes from tests/diffuse_ref.py, tests/diffuse_solve_ref.py and tests/spectral_ref.py on `gl.to_csr()`, in
bits, or is one of the bounds of tests/test_gpu_spectral.py.  Every test asserts the counts that make it reach its path, so a
smaller shape fails instead of passing for nothing.  tests/test_spectral_inputs.py and tests/test_diffuse_solve_inputs.py show
shape C's properties on the CPU; shapes L and M are too large for the numpy oracle and their test states what it leans on from
the reference over the device's CSR, before it looks at the device's answer.  Both are built by the ordinary
`ArrowSpaceBuilder.build` (half a second on the MI355X)."""
import ctypes as C
import struct
import threading
import time

import numpy as np
import pytest

import diffuse_ref as dfr
import diffuse_solve_ref as dsr
import spectral_ref as spr
from test_gpu_diffuse import index, tune
from test_gpu_diffuse_solve import same_solve
from test_gpu_spectral import MAX_ITERS, TOL, counters as eigs_counters, same_bits, solver_checks

pytestmark = pytest.mark.gpu

TAU = dfr.TAU
MIB = 1 << 20
GRAM_STRANDS = 1024 // 64     # strands per entry of the Gram's tree: its 1 024 threads over the 64 entries of a block
NORM_STRANDS = 1024 // 4      # and of the column norms' tree: four entries per block
SOLVE_STRANDS = 1024          # threads of the solve's tree: one block per column
GRID_BLOCKS_PER_CU = 8        # the uncapped grid: blocks per compute unit, of four waves each
_tree = {}


def pow2(v):
    p = 1
    while p < v:
        p *= 2
    return p


def same(a, b):
    """Equal in bits, through tuples, lists and dicts."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return struct.pack("d", a) == struct.pack("d", b)
    return a == b


def tree_blocks(n, cols):
    """The hand-made blocks of the tree test and the reference of the four results: once per (n, C), not once per grid cap."""
    if (n, cols) not in _tree:
        A, B = spr.hand_block(n, cols, 31), spr.hand_block(n, cols, 32)
        T = spr.hand_block(cols, cols, 33)
        theta = np.random.default_rng(34).uniform(-1.0, 1.0, cols) * 10.0 ** np.random.default_rng(35).uniform(-3.0, 3.0, cols)
        want = {"gram": spr.gram(A, B), "gram2": spr.gram(A, A), "rotate": spr.rotate(A, T), "colnorm2": spr.colnorm2(A, B, theta)}
        _tree[(n, cols)] = (A, B, T, theta, want)
    return _tree[(n, cols)]


@pytest.mark.parametrize("cols", [16, 64])
@pytest.mark.parametrize("n", [32768, 33797, 60421])
def test_the_trees_past_one_trip_of_their_strands(n, cols):
    ix = index("A")
    gseg, dseg = -(-n // spr.GRAM_SEG), -(-n // dsr.SEG)
    if n == 33797:
        # a level of more pairs than two trips of the strands start, in trees with pairs whose upper half lies past the last segment
        assert (gseg, dseg) == (34, 529)
        assert gseg > 2 * GRAM_STRANDS and dseg > 2 * NORM_STRANDS
        assert (pow2(gseg), pow2(dseg)) == (64, 1024) and gseg - 32 < 32 and dseg - 512 < 512
        assert n % 16 == n % 64 == n % 1024 == 5
    elif n == 60421:
        # at 33 797 rows the pairs of the second trip (16 .. 31 of 32, 256 .. 511 of 512) all add padding, so a strand that skips
        # one of them returns the same bits; here 12 and 177 of them add a partial that exists, the others padding
        assert (gseg, dseg) == (60, 945) and (pow2(gseg), pow2(dseg)) == (64, 1024)
        assert gseg - 32 - GRAM_STRANDS == 12 and dseg - 512 - NORM_STRANDS == 177
        assert n % 16 == n % 64 == n % 1024 == 5
    else:
        # the last size of one trip: 2 x 16 and 2 x 256 segments, no padding anywhere
        assert (gseg, dseg) == (32, 512) == (2 * GRAM_STRANDS, 2 * NORM_STRANDS) == (pow2(gseg), pow2(dseg))
        assert n % 1024 == 0
    A, B, T, theta, want = tree_blocks(n, cols)
    assert (dfr.canon(want["gram"]) != dfr.canon(A.T @ B)).any()   # (a changed order changes bits)
    try:
        for cap in (0, 1):
            tune(ix, {b"diffuse_grid_cap": cap})
            same_bits(ix.aspace._spectral_op(ix.gl, "gram", A, B), want["gram"], (cap, "gram"))
            same_bits(ix.aspace._spectral_op(ix.gl, "gram", A), want["gram2"], (cap, "gram of a block with itself"))
            same_bits(ix.aspace._spectral_op(ix.gl, "rotate", A, T=T), want["rotate"], (cap, "rotate"))
            same_bits(ix.aspace._spectral_op(ix.gl, "colnorm2", A, B, T=theta), want["colnorm2"], (cap, "colnorm2"))
    finally:
        tune(ix, {})


@pytest.mark.parametrize("name", ["L", "M"])
def test_the_solves_tree_and_the_uncapped_grid(name):
    t0 = time.perf_counter()
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    print(f"{name}: torch and its device properties {time.perf_counter() - t0:.2f} s")
    t0 = time.perf_counter()
    ix = index(name)
    print(f"{name}: build, to_csr() and the operator {time.perf_counter() - t0:.2f} s")
    aspace, gl, n = ix.aspace, ix.gl, ix.n
    nseg = -(-n // dsr.SEG)
    assert n - dsr.SEG * (nseg - 1) == 1            # one row in the last segment
    assert nseg > 2 * SOLVE_STRANDS                 # the first level of the solve's tree has more pairs than its block has threads
    if name == "L":
        # the smallest such n; the pairs of the second trip (1 024 .. 2 047) all add padding (segments 3 072 and up)
        assert (n, nseg) == (131137, 2050) and pow2(nseg) == 4096
    else:
        # 528 pairs of the second trip add a partial that exists: a thread that skips one of them changes the sum
        assert (n, nseg) == (230337, 3600) and pow2(nseg) == 4096 and nseg - 2048 - SOLVE_STRANDS == 528
    trip = cus * GRID_BLOCKS_PER_CU * 16            # rows of one trip of the uncapped grid at 16 columns: four waves of four rows a block
    assert n > trip, f"{cus} compute units: the shape must grow beyond {trip} rows to wrap the grid"
    seeds = dsr.seed_columns(n, ix.gp["topk"], count=3)
    edge = [bool((ix.deg[ids] > 0).any()) for ids, _ in seeds]
    assert sum(edge) >= 2
    Y = np.stack([dfr.seeds_vector(n, i, v) for i, v in seeds], axis=1)
    # the CPU reference first, and what the check leans on
    t0 = time.perf_counter()
    want = dsr.solve(*ix.op, Y, 0.5, 1e-6, 100)
    step = dfr.diffuse(*ix.op, Y, 0.5, 2)
    print(f"{name}: {int((ix.deg == 0).sum())} rows without an edge, the longest row {int(ix.deg.max())}; seeds with an edge {edge}; the reference: "
          f"iterations {want[1].tolist()}, residuals {want[2].tolist()}, {time.perf_counter() - t0:.2f} s")
    for c in range(3):
        if edge[c]:
            assert want[3][c] and want[1][c] >= 3
    assert all(np.count_nonzero(step[:, c]) > len(seeds[c][0]) for c in range(3) if edge[c])   # (the recurrence moves something)
    t0 = time.perf_counter()
    try:
        tune(ix, {})
        # three columns run as one 16-wide chunk; then one column alone
        got, info = aspace.diffuse_solve(gl, seeds, 0.5, 1e-6)
        same_solve(got, info, want, [0, 1, 2], "a 16-wide chunk")
        one = edge.index(True)
        got, info = aspace.diffuse_solve(gl, [seeds[one]], 0.5, 1e-6)
        same_solve(got, info, want, [one], "one column")
        # the recurrence at the real grid: more rows than one trip
        got = aspace.diffuse(gl, seeds, 0.5, 2)
        assert got.shape == (3, n) and (dfr.canon(got) == dfr.canon(step.T)).all()
        print(f"{name}: the three device calls and their comparisons {time.perf_counter() - t0:.2f} s")
    finally:
        tune(ix, {})


def multiplicity_checks(m, values, lam):
    """Shape C: the value 1 has multiplicity 19 and the next value lies a gap of more than 1e-3 below."""
    assert (np.abs(lam[:19] - 1.0) <= TOL).all() and lam[19] < 1.0 - 1e-3
    assert (np.abs(values[:min(m, 19)] - 1.0) <= TOL).all()      # no copy missed, none counted twice
    if m > 19:
        assert values[19] < 1.0 - 1e-3


@pytest.mark.parametrize("m, cols", spr.SCALE_CASES)
def test_eigsh_on_shape_c(m, cols):
    ix = index("C")
    assert ix.n == 2053 and -(-ix.n // spr.GRAM_SEG) == 3 and -(-ix.n // dsr.SEG) == 33   # three Gram partials in every sum
    assert (ix.deg == 0).any() and ix.deg.max() >= 24
    values, vectors, info, lam = solver_checks("C", m, cols)
    multiplicity_checks(m, values, lam)


def test_eigsh_on_shape_c_under_two_grids():
    ix = index("C")
    u = lambda a: a.view(np.uint64)   # noqa: E731
    try:
        v0, x0, i0 = ix.aspace.eigsh(ix.gl, 13, TOL, MAX_ITERS, with_info=True)
        tune(ix, {b"diffuse_grid_cap": 1})
        v1, x1, i1 = ix.aspace.eigsh(ix.gl, 13, TOL, MAX_ITERS, with_info=True)
        assert (u(v0) == u(v1)).all() and (u(x0) == u(x1)).all() and (u(i0["residuals"]) == u(i1["residuals"])).all()
        assert i0["converged"] and {k: v for k, v in i0.items() if k != "residuals"} == {k: v for k, v in i1.items() if k != "residuals"}
    finally:
        tune(ix, {})


def test_the_budgets_choose_the_chunk_width():
    ix = index("C")
    asp, aspace, gl, n = ix.asp, ix.aspace, ix.gl, ix.n
    col = 8 * n   # bytes of a column of one buffer
    assert 2 * col * 64 > 1 * MIB >= 2 * col * 16                     # the recurrence's two buffers under 1 MiB: 16 columns
    assert 4 * col * 16 > 1 * MIB                                     # the solve's four vectors under 1 MiB: one column
    assert 4 * col * 64 > 2 * MIB >= 4 * col * 16                     # and under 2 MiB: 16 columns
    seeds = dsr.seed_columns(n, ix.gp["topk"], count=40)
    assert len(seeds) == 40 > 32                                      # (the default budget takes 64 columns)
    Y = np.stack([dfr.seeds_vector(n, i, v) for i, v in seeds], axis=1)
    want_step = dfr.diffuse(*ix.op, Y, 0.85, 3).T
    want = dsr.solve(*ix.op, Y, 0.85, 1e-10, 100)
    it = want[1]
    assert want[3].all() and len(set(it.tolist())) >= 3               # (tests/test_diffuse_solve_inputs.py)
    assert {"column chunks"} <= set(aspace.diffuse_counters()) and {"column chunks", "iterations launched"} <= set(aspace.diffuse_solve_counters())
    by16 = int(it[:16].max() + it[16:32].max() + it[32:].max())
    try:
        tune(ix, {})
        first = None
        for mib, chunks in ((0, 1), (1, 3)):                          # 64 columns; 16 + 16 + 8
            assert asp._L.as_set_tuning(b"diffuse_mib", mib) == 0
            c0 = aspace.diffuse_counters()
            got = aspace.diffuse(gl, seeds, 0.85, 3)
            c1 = aspace.diffuse_counters()
            assert (dfr.canon(got) == dfr.canon(want_step)).all(), mib
            first = got if first is None else first
            assert (got.view(np.uint64) == first.view(np.uint64)).all(), mib
            assert c1["column chunks"] - c0["column chunks"] == chunks, mib
            assert c1["step launches"] - c0["step launches"] == 3 * chunks, mib
        assert asp._L.as_set_tuning(b"diffuse_mib", 0) == 0
        first = None
        for mib, chunks, launched in ((0, 1, int(it.max())), (2, 3, by16), (1, 40, int(it.sum()))):   # 64 columns; 16 + 16 + 8; 40 x 1
            assert asp._L.as_set_tuning(b"diffuse_solve_mib", mib) == 0
            c0 = aspace.diffuse_solve_counters()
            got, info = aspace.diffuse_solve(gl, seeds, 0.85, 1e-10)
            c1 = aspace.diffuse_solve_counters()
            same_solve(got, info, want, list(range(40)), mib)
            first = (got, info) if first is None else first
            assert same((got, info), first), mib
            assert c1["column chunks"] - c0["column chunks"] == chunks, mib
            assert c1["iterations launched"] - c0["iterations launched"] == launched, mib
    finally:
        assert asp._L.as_set_tuning(b"diffuse_mib", 0) == 0
        assert asp._L.as_set_tuning(b"diffuse_solve_mib", 0) == 0
        tune(ix, {})


def test_timing_mode_changes_no_bit():
    ix = index("B")
    asp, aspace, gl = ix.asp, ix.aspace, ix.gl
    L = asp._L
    assert L.as_graph_eigs_kernel_us.restype is C.c_double and L.as_diffuse_solve_kernel_us.restype is C.c_double
    eig_us = lambda part: L.as_graph_eigs_kernel_us(aspace._h, part)        # noqa: E731
    sol_us = lambda part: L.as_diffuse_solve_kernel_us(aspace._h, part)     # noqa: E731
    seeds = dsr.seed_columns(ix.n, ix.gp["topk"])[:20]
    Y = np.stack([dfr.seeds_vector(ix.n, i, v) for i, v in seeds], axis=1)

    def eig(m):
        c0 = eigs_counters(ix)
        out = aspace.eigsh(gl, m, TOL, MAX_ITERS, with_info=True)
        return out, [a - b for a, b in zip(eigs_counters(ix), c0)]

    def solve(max_iters):
        c0 = aspace.diffuse_solve_counters()
        out = aspace.diffuse_solve(gl, seeds, 0.85, 1e-10, max_iters=max_iters)
        c1 = aspace.diffuse_solve_counters()
        return out, {k: c1[k] - c0[k] for k in c1}

    plain = {("eig", m): eig(m) for m in (8, 19)}
    plain.update({("solve", mi): solve(mi) for mi in (100, 1)})
    for mi in (100, 1):   # the untimed answers are the reference's
        same_solve(*plain[("solve", mi)][0], dsr.solve(*ix.op, Y, 0.85, 1e-10, mi), list(range(20)), mi)
    assert plain[("solve", 100)][0][1]["iterations"].min() >= 2           # every chunk has a second iteration: the one that is sampled
    assert plain[("solve", 1)][0][1]["iterations"].tolist() == [1] * 20    # and the only one under max_iters = 1
    try:
        assert L.as_set_tuning(b"diffuse_timing", 1) == 0
        for m in (8, 19):
            timed = eig(m)
            assert same(timed, plain[("eig", m)]), m
            assert timed[1][0] == 1 and timed[1][1] == timed[0][2]["iterations"]
            assert all(eig_us(part) > 0.0 for part in range(5)), [eig_us(part) for part in range(7)]   # the call; step, gram, rotate, colnorm2
            assert eig_us(5) >= 0.0 and eig_us(6) >= 0.0               # the host's decompositions and waits
            assert eig_us(-1) == 0.0 and eig_us(7) == 0.0
        for mi in (100, 1):   # the second iteration of a chunk is sampled, or the only one
            timed = solve(mi)
            assert same(timed, plain[("solve", mi)]), mi
            assert timed[1]["column chunks"] == 2 and timed[1]["calls"] == 1
            assert all(sol_us(part) > 0.0 for part in range(6)), (mi, [sol_us(part) for part in range(6)])
            assert sol_us(-1) == 0.0 and sol_us(6) == 0.0
    finally:
        assert L.as_set_tuning(b"diffuse_timing", 0) == 0
    # the driver zeroes its timers per call: an untimed call leaves none of the launches' behind
    assert same(eig(8), plain[("eig", 8)])
    assert [eig_us(part) for part in (1, 2, 3, 4)] == [0.0] * 4


def test_two_host_threads_on_the_solve_and_the_eigenpairs():
    ix = index("B")
    aspace, gl = ix.aspace, ix.gl
    seeds = dsr.seed_columns(ix.n, ix.gp["topk"])[:20]
    Q = ix.queries(np.random.default_rng(53), 4)
    jobs = [lambda: aspace.eigsh(gl, 8, TOL, MAX_ITERS, with_info=True),
            lambda: aspace.eigsh(gl, 19, TOL, MAX_ITERS, with_info=True),
            lambda: aspace.diffuse_solve(gl, seeds, 0.85, 1e-10),
            lambda: [aspace.search_diffuse_solve(q, gl, TAU, 0.85, 1e-8, with_info=True) for q in Q],
            lambda: aspace.diffuse(gl, seeds, 0.85, 3)]
    serial = [job() for job in jobs]
    assert serial[0][2]["converged"] and serial[1][2]["converged"] and serial[2][1]["converged"].all()
    assert all(info["converged"] and info["iterations"] >= 5 for _, info in serial[3])
    errors = []

    def run(order):
        try:
            for j in order:
                assert same(jobs[j](), serial[j]), j
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=run, args=(order,)) for order in (range(5), range(4, -1, -1))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]
