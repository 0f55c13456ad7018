"""The HIP two-stage refine path (byte first pass -> top-R -> exact f32
re-rank -> top-k) against the CPU reference in oracle/refine.py, at the tile
widths, dims, metrics, depths and tie patterns listed in
tests/refine_cases.py. Every search with refine on runs FIRST on a fresh
index: a prior search over the same queries leaves correct values in the
reused candidate buffer and hides unscanned tile lanes.

Kernel instantiations reached:
  scan_i8_dot_kernel<*, false, 16>  dims 16 48 64 768 (L2SQ IP COS L1),
                                    3056 (L2SQ IP)
  scan_i8_dot_kernel<*, false, 8>   dim 3072 (16*dpad+80 > 48 KiB; L2SQ IP)
  scan_i8_kernel<*, false>          dims 100 and 67 (dpad % 16 != 0; all 4)
  refine_kernel<L2SQ|IP|COS|L1>, compose_select_kernel, gather (sqrt for l2)
  topk_kernel: whole-bin exit, boundary-group collect, level-3 tie mode
  (ties-flood), count <= k copy (short lists)."""

import numpy as np
import pytest

import refine_cases as rc
from oracle import refine as rf

pytestmark = pytest.mark.gpu


def _names(prefix):
    return [c.name for c in rc.CASES if c.name.startswith(prefix)]


def _fresh_index(c):
    from matrixone_amd import engine
    cp = rc.corpus(c.kind, c.d)
    ix = engine.IvfFlatIndex(c.d, rc.NLIST, metric=c.metric,
                             capacity=cp.vecs.shape[0])
    ix.add(cp.vecs, ids=cp.ids)
    ix.set_centroids(cp.cents)
    ix.set_assignments(cp.assign.astype(np.int32))
    ix.build()
    return ix


def _check(c, ids, dists, allowed=None, ctx=""):
    skipped, n_must = rf.check_two_stage(
        ids, dists, rc.reference(c), c.k, c.R, allowed=allowed,
        ctx=f"{c.name}{ctx}")
    print(f"{c.name}{ctx}: skipped {skipped} of {n_must} must candidates")
    assert skipped <= rc.SKIP_CAP * n_must, (c.name, skipped, n_must)


def _assert_exact_parity(c, ids, dists):
    """R >= every candidate count: the result must equal the plain exact
    search of the oracle (ids bit-exact except at FP ties)."""
    from test_parity_gpu import _assert_parity
    cp = rc.corpus(c.kind, c.d)
    om, orig_l2 = rc.METRICS[c.metric]
    ref_ids, ref_d = cp.idx.search(om, rc.queries(c), c.probe, c.k,
                                   orig_l2=orig_l2)
    np.testing.assert_array_equal(ids == -1, ref_ids == -1, err_msg=c.name)
    _assert_parity(ids, dists, ref_ids, ref_d, ctx=c.name)


def _run_case(c):
    ix = _fresh_index(c)
    try:
        ix.enable_refine(c.depth)
        ids, dists = ix.search(rc.queries(c), c.k, c.probe)
    finally:
        ix.close()
    if c.depth >= 4096:
        _assert_exact_parity(c, ids, dists)
    _check(c, ids, dists)


@pytest.mark.parametrize("name", _names("tile-"))
def test_tile_geometry(name):
    """probe = nlist: every non-empty list sees all nq queries, so nq sets
    the tile shapes (single, half, full, tails below/at/above 8, several
    tiles); tile-mixed puts {1, 8, 9, 16, 17, 40} queries on six lists of
    one launch."""
    _run_case(rc.BY_NAME[name])


@pytest.mark.parametrize("name", _names("md-") + _names("big-"))
def test_metrics_and_dims(name):
    """Every metric x dims with d16 in {1, 3, 4, 48}, the uchar4 fallback
    (100, 67) and the two sides of the QT=16 LDS limit (3056, 3072); at full
    depth the result is the exact search, at depth 32 the band contract."""
    _run_case(rc.BY_NAME[name])


@pytest.mark.parametrize("name", ["rk-k50-depth8", "rk-k1", "rk-depth10",
                                  "rk-k200-depth4096"])
def test_depth_and_k(name):
    """k > depth (R = k), k = 1, R not a multiple of the 4 waves, and a
    large k under full depth."""
    _run_case(rc.BY_NAME[name])


def test_disable_and_reenable():
    """enable_refine(0) returns to the exact scan; re-enabling at another
    depth reuses the byte image."""
    c32 = rc.BY_NAME["tile-d64-nq25"]
    c16 = rc.BY_NAME["rk-reenable-depth16"]
    q = rc.queries(c32)
    assert np.array_equal(q, rc.queries(c16))
    ix = _fresh_index(c32)
    ix.enable_refine(c32.depth)
    ids, dists = ix.search(q, c32.k, c32.probe)
    _check(c32, ids, dists)
    ix.enable_refine(0)
    ids, dists = ix.search(q, c32.k, c32.probe)
    _assert_exact_parity(c32, ids, dists)
    ix.enable_refine(c16.depth)
    ids, dists = ix.search(q, c16.k, c16.probe)
    ix.close()
    _check(c16, ids, dists)


@pytest.mark.parametrize("name", ["filt-rate30", "filt-lists"])
def test_filtered(name):
    """search_filtered with refine on; filt-lists has queries with fewer
    than R, fewer than k and no passing candidates."""
    c = rc.BY_NAME[name]
    cp = rc.corpus(c.kind, c.d)
    allowed = rc.allowed_rows(c)
    ref = rc.reference(c)
    npass = np.array([int(allowed[r].sum()) for r in ref.cand_rows])
    if name == "filt-lists":
        assert (npass == 0).any() and ((npass > 0) & (npass < c.k)).any() \
            and ((npass >= c.k) & (npass < c.R)).any() and (npass > c.R).any()
    ix = _fresh_index(c)
    ix.enable_refine(c.depth)
    ids, dists = ix.search_filtered(rc.queries(c), c.k, c.probe,
                                    ix.filter_bitset(cp.ids[allowed]))
    ix.close()
    _check(c, ids, dists, allowed=allowed)


def test_soft_delete():
    """delete_id of every id that ranks first, then search again: they are
    gone and the contract holds over the remaining rows."""
    c = rc.BY_NAME["delete-top1"]
    q = rc.queries(c)
    ix = _fresh_index(c)
    ix.enable_refine(c.depth)
    ids, dists = ix.search(q, c.k, c.probe)
    _check(c, ids, dists, ctx=" before")
    gone = np.unique(ids[:, 0])
    for i in gone:
        ix.delete_id(int(i))
    ids, dists = ix.search(q, c.k, c.probe)
    ix.close()
    assert not np.isin(ids, gone).any()
    _check(c, ids, dists, allowed=rc.mask_without_ids(c, gone),
           ctx=" after delete")


@pytest.mark.parametrize("name", ["ties-dup4", "ties-flood"])
def test_byte_distance_ties(name):
    """Every vector x4, and 1500 identical rows in one list: for the queries
    next to them the boundary tie group (1500 equal keys) exceeds the
    1024-key sort buffer, so the radix select ends in its level-3 tie mode,
    where atomic order picks the ids. Ids inside the band are free; the
    count, the distances and everything outside the band are not. Distances
    must repeat from run to run (ids need not: see DESIGN.md)."""
    c = rc.BY_NAME[name]
    if name == "ties-flood":
        ref = rc.reference(c)
        b = ref.bdist[0]
        assert (b == b.min()).sum() == rc.FLOOD_ROWS > 1024
    ix = _fresh_index(c)
    ix.enable_refine(c.depth)
    ids, dists = ix.search(rc.queries(c), c.k, c.probe)
    ids2, dists2 = ix.search(rc.queries(c), c.k, c.probe)
    ix.close()
    _check(c, ids, dists)
    _check(c, ids2, dists2, ctx=" rerun")
    print(f"{name}: ids repeat across runs: {np.array_equal(ids, ids2)}")
    np.testing.assert_array_equal(dists, dists2)


def test_pipelined_submit_collect():
    """The path the benchmark times: device batches of {33, 1, 16, 25, 33}
    queries through search_submit/search_collect at pipeline depth 2, refine
    on; every collected result meets the contract against its own queries,
    also in a second round on the reused contexts."""
    import torch
    cases = [rc.BY_NAME[n] for n in _names("pipe-")]
    assert [c.nq for c in cases] == [33, 1, 16, 25, 33]
    c0 = cases[0]
    ix = _fresh_index(c0)
    ix.enable_refine(c0.depth)
    batches = [torch.from_numpy(rc.queries(c)).cuda() for c in cases]
    torch.cuda.synchronize()
    for rnd in range(2):
        tickets, got = [], []
        for qb in batches:
            tickets.append(ix.search_submit(qb, c0.k, c0.probe))
            if len(tickets) == 2:
                got.append(ix.search_collect(tickets.pop(0)))
        while tickets:
            got.append(ix.search_collect(tickets.pop(0)))
        for c, (ids, dists) in zip(cases, got):
            _check(c, ids, dists, ctx=f" round {rnd}")
    ix.close()
