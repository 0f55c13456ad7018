"""The fused refine tail (refine_finish_kernel) and the threshold-filter
selection inside the search, against the kernels they replace: on ONE index
the same search runs with the legacy tail (radix select, refine_kernel ->
topk_kernel -> compose_select_kernel -> gather_kernel) and with the default
one, and ids and distance bits must be identical. The exact distances keep
refine_kernel's per-lane summation order, so there is no tolerance.

Corpora and queries are those of tests/refine_cases.py (the `flood` corpus
is left out: its ids are free by design). Reached: dims 16, 100 (row tail
shorter than a wave) and 768, all five metrics (l2 for the sqrt write-out),
depth 10 (not a multiple of 4 waves x 4 candidates), 32, 64, 1024 (the
largest fused R) and 1025 (the old chain on both sides), k 1 / 10 / 50 over
depth 8 (R = k), queries with no / fewer than k / fewer than R passing
candidates, and the submit/collect path at depth 2. A last test makes every
query see 20 000 candidates, where the filter selection engages."""

import numpy as np
import pytest

import refine_cases as rc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(c):
    from matrixone_amd import engine
    cp = rc.corpus(c.kind, c.d)
    ix = engine.IvfFlatIndex(c.d, rc.NLIST, metric=c.metric,
                             capacity=cp.vecs.shape[0])
    ix.add(cp.vecs, ids=cp.ids)
    ix.set_centroids(cp.cents)
    ix.set_assignments(cp.assign.astype(np.int32))
    ix.build()
    ix.enable_refine(c.depth)
    return ix


def _both_tails(ix, search):
    """search() under the legacy tail, then under the default one."""
    out = []
    for legacy in (True, False):
        ix.set_refine_tail(legacy)
        out.append(search())
    return out


def _assert_same(old, new, ctx):
    np.testing.assert_array_equal(new[0], old[0], err_msg=f"{ctx} ids")
    np.testing.assert_array_equal(_bits(new[1]), _bits(old[1]),
                                  err_msg=f"{ctx} dists")


def _compare(c):
    ix = _index(c)
    try:
        q = rc.queries(c)
        old, new = _both_tails(ix, lambda: ix.search(q, c.k, c.probe))
    finally:
        ix.close()
    _assert_same(old, new, c.name)
    assert (new[0][:, 0] >= 0).any(), c.name
    return new


@pytest.mark.parametrize("metric", list(rc.METRICS))
@pytest.mark.parametrize("d", [16, 100, 768])
def test_metrics_and_dims(metric, d):
    _compare(rc.BY_NAME[f"md-{metric}-d{d}-R32"])


@pytest.mark.parametrize("depth", [10, 64, 1024, 1025])
def test_depths(depth):
    if depth == 10:
        c = rc.BY_NAME["rk-depth10"]
    else:
        c = rc.Case(f"finish-depth{depth}", 100, "l2sq", 25, depth=depth)
    ids, _ = _compare(c)
    assert (ids >= 0).all()


@pytest.mark.parametrize("name", ["rk-k1", "rk-k50-depth8"])
def test_k(name):
    _compare(rc.BY_NAME[name])


def test_filtered_queries_short_of_k_and_r():
    """filt-lists: queries with no passing candidate, fewer than k and fewer
    than R; the padding of both tails must agree entry for entry."""
    c = rc.BY_NAME["filt-lists"]
    cp = rc.corpus(c.kind, c.d)
    allowed = rc.allowed_rows(c)
    ix = _index(c)
    try:
        bits = ix.filter_bitset(cp.ids[allowed])
        old, new = _both_tails(
            ix, lambda: ix.search_filtered(rc.queries(c), c.k, c.probe, bits))
    finally:
        ix.close()
    _assert_same(old, new, c.name)
    npass = (new[0] >= 0).sum(axis=1)
    assert (npass == 0).any() and ((npass > 0) & (npass < c.k)).any() \
        and (npass == c.k).any()
    assert (new[1][new[0] < 0] == np.finfo(np.float32).max).all()


def test_pipelined_submit_collect():
    """Device batches of {33, 1, 16, 25, 33} queries through
    search_submit/search_collect at pipeline depth 2, both tails."""
    import torch
    cases = [c for c in rc.CASES if c.name.startswith("pipe-")]
    c0 = cases[0]
    ix = _index(c0)
    batches = [torch.from_numpy(rc.queries(c)).cuda() for c in cases]
    torch.cuda.synchronize()

    def run():
        tickets, got = [], []
        for qb in batches:
            tickets.append(ix.search_submit(qb, c0.k, c0.probe))
            if len(tickets) == 2:
                got.append(ix.search_collect(tickets.pop(0)))
        while tickets:
            got.append(ix.search_collect(tickets.pop(0)))
        return got

    try:
        old, new = _both_tails(ix, run)
    finally:
        ix.close()
    for c, o, n in zip(cases, old, new):
        _assert_same(o, n, c.name)


@pytest.mark.parametrize("depth", [64, 0])
def test_filter_selection_inside_the_search(depth):
    """Four lists of 5 000 rows, all probed: every query selects from 20 000
    candidates, past the filter's engage count, for the refine top-R
    (depth 64) and for the exact path's top-k (depth 0). Same ids and bits as
    the radix select, and select_stats accounts for every query."""
    from matrixone_amd import engine
    rng = np.random.Generator(np.random.PCG64(20000 + depth))
    n, d, nlist, nq, k = 20000, 16, 4, 24, 10
    vecs = rng.standard_normal((n, d), dtype=np.float32)
    cents = rng.standard_normal((nlist, d), dtype=np.float32)
    assign = (np.arange(n) % nlist).astype(np.int32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    assert engine.select_plan(n, max(k, depth))["filter"]
    ix = engine.IvfFlatIndex(d, nlist, metric="l2sq", capacity=n)
    try:
        ix.add(vecs, ids=np.arange(n, dtype=np.int64) + 7)
        ix.set_centroids(cents)
        ix.set_assignments(assign)
        ix.build()
        if depth:
            ix.enable_refine(depth)
        old, new = _both_tails(ix, lambda: ix.search(q, k, nlist))
        st = ix.select_stats()
    finally:
        ix.close()
    _assert_same(old, new, f"filter-depth{depth}")
    assert (new[0] >= 0).all()
    print(f"depth {depth}: select_stats {st}")
    assert st["filtered"] + st["fallback"] == nq
    assert st["fallback"] <= 1
