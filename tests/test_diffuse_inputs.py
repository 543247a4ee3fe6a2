"""CPU: the inputs of tests/test_gpu_diffuse.py have the properties its checks lean on, shown on the numpy oracle's build of the
same items: every shape has a row without an edge, a longest row of at least three tiles of the "diffuse_tile_edges" the GPU
test sets (so a row's sum is carried across tiles), a number of items that is no multiple of 64 (the last wave and the last row
group are partial) and more than one row group; and for consequence (a) of S19 a query whose pool is full with every score > 0."""
import numpy as np
import pytest

import diffuse_ref as dfr
from oracle import oracle_np


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_the_gpu_shapes_have_the_rows_the_kernels_must_survive(name):
    X, gp = dfr.shape_items(name)
    n = X.shape[0]
    idx = oracle_np.build(X, gp)
    deg = np.diff(idx["indptr"])
    print(f"{name}: n {n}, edges {int(idx['indptr'][-1])}, longest row {int(deg.max())}, rows without an edge {int((deg == 0).sum())}")
    assert (deg == 0).sum() >= 1
    assert deg.max() >= 3 * dfr.TILE_EDGES
    assert n % 64 != 0 and n > 256
    # the oracle's rows are what the reference reads through to_csr(): columns ascending, no diagonal stored
    rows = np.repeat(np.arange(n), deg)
    assert (idx["indices"] != rows).all()
    for i in range(n):
        assert (np.diff(idx["indices"][idx["indptr"][i]:idx["indptr"][i + 1]]) > 0).all()


@pytest.mark.parametrize("name", list(dfr.SHAPES))
def test_full_pools_with_positive_scores(name):
    X, gp = dfr.shape_items(name)
    idx = oracle_np.build(X, gp)

    def served(q):
        try:
            oracle_np.search(idx, q, dfr.TAU)
            return True
        except oracle_np.ZeroLambda:
            return False

    for q in dfr.queries_of(X, np.random.default_rng(5), dfr.NQ, served):
        hits, _ = oracle_np.search(idx, q, dfr.TAU)
        assert len(hits) == gp["topk"] and min(v for _, v in hits) > 0.0
