"""GPU parity at the graph and row-width edges: the CDNA4 HNSW beam kernel
against the numpy oracle on every case of tests/hnsw_cases.py (hand-built
graphs bit for bit, engine-built ones inside the suite's distance band),
plus the host paths around it: workspace reuse on one handle, device-resident
queries, the eval counter, errors, the l2 transform and the multi-model
merge. tests/test_hnsw_cases_ref.py proves on the CPU that these comparisons
reject the kernel errors the cases are in the table for."""

import numpy as np
import pytest

import hnsw_cases as hc
from oracle import hnsw as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def index_of():
    """One device index per graph, shared by the tests of this file."""
    from matrixone_amd.hnsw import HnswIndex
    cache = {}

    def get(c):
        if c.graph not in cache:
            cache[c.graph] = HnswIndex(hc.graph_data(hc.graph(c)))
        return cache[c.graph]

    yield get
    for ix in cache.values():
        ix.close()


def _search(ix, c, qs=None):
    qs = hc.queries(c) if qs is None else qs
    if c.filtered:
        return ix.search_filtered(qs, c.ef, c.k,
                                  hc.slot_bitset(hc.pass_slots(c)))
    return ix.search(qs, c.ef, c.k)


def _run(index_of, name):
    c = hc.BY_NAME[name]
    ids, d = _search(index_of(c), c)
    ref_ids, ref_d = hc.reference(c)
    print(f"{name}: gpu ids[0]={ids[0][:8].tolist()} d[0]={d[0][:4].tolist()}"
          f" ref ids[0]={ref_ids[0][:8].tolist()}")
    excused = hc.check(c, ids, d, ref_ids, ref_d)
    print(f"{name}: excused {excused} of {ids.size}")


# ------------------------------------------------------------- case runs

@pytest.mark.parametrize("name", hc.names("chains"))
def test_chains(index_of, name):
    """A level-0 path with more hops than any expansion bound short of n."""
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("degenerate"))
def test_degenerate(index_of, name):
    """n = 1, k > n, ef > n, max_level 0, an entry with no neighbours, an
    unreachable component."""
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("stars"))
def test_stars(index_of, name):
    """Sort widths 512 and 2048, more than 1024 neighbours, kept > ef."""
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("tower"))
def test_tower(index_of, name):
    """Three 16-wide descent rounds, equal-distance decoys, 30 re-scans."""
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("ties"))
def test_ties(index_of, name):
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("wide"))
def test_wide(index_of, name):
    """Rows of 65, 192 and 257 quads: the lane loop's stride and tail."""
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("tiny"))
def test_tiny(index_of, name):
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("degree"))
def test_degree(index_of, name):
    _run(index_of, name)


@pytest.mark.parametrize("name", hc.names("filtered"))
def test_filtered(index_of, name):
    c = hc.BY_NAME[name]
    _run(index_of, name)
    ids, _ = _search(index_of(c), c)
    g = hc.graph(c)
    ok = set(int(x) for x in g.keys[hc.pass_slots(c)])
    assert all(int(x) in ok for x in ids[ids >= 0]), "filtered-out id"


@pytest.mark.parametrize("name", [c.name for c in hc.CASES])
def test_deterministic(index_of, name):
    c = hc.BY_NAME[name]
    a = _search(index_of(c), c)
    b = _search(index_of(c), c)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ------------------------------------------------------- one handle, reused

def test_workspace_reuse_and_device_queries():
    """nq 16 -> 3 -> 16, then filtered, then unfiltered on ONE handle: each
    call equals the same call on a fresh handle, bitwise; device-resident
    queries equal host ones."""
    import torch

    from matrixone_amd.hnsw import HnswIndex
    c = hc.BY_NAME[hc.REUSE_CASE]
    gd = hc.graph_data(hc.graph(c))
    qs = hc.queries(c)
    assert len(qs) == 16
    n = len(gd.levels)
    rng = np.random.Generator(np.random.PCG64(5))
    bits = hc.slot_bitset(rng.random(n) < 0.5)

    def fresh(fn):
        ix = HnswIndex(gd)
        try:
            return fn(ix)
        finally:
            ix.close()

    def same(a, b, what):
        np.testing.assert_array_equal(a[0], b[0], err_msg=what)
        np.testing.assert_array_equal(a[1].view(np.uint32),
                                      b[1].view(np.uint32), err_msg=what)

    one16 = fresh(lambda ix: ix.search(qs, c.ef, c.k))
    one3 = fresh(lambda ix: ix.search(qs[5:8], c.ef, c.k))
    onef = fresh(lambda ix: ix.search_filtered(qs, c.ef, c.k, bits))
    hc.check(c, *one16, *hc.reference(c))
    same(one3, (one16[0][5:8], one16[1][5:8]), "a query's batch matters")

    ix = HnswIndex(gd)
    same(ix.search(qs, c.ef, c.k), one16, "nq 16")
    same(ix.search(qs[5:8], c.ef, c.k), one3, "nq 3 after 16")
    same(ix.search(qs, c.ef, c.k), one16, "nq 16 after 3")
    same(ix.search_filtered(qs, c.ef, c.k, bits), onef, "filtered")
    same(ix.search(qs, c.ef, c.k), one16, "unfiltered after filtered")
    same(ix.search_filtered(qs, c.ef, c.k, bits), onef, "filtered again")
    qt = torch.from_numpy(qs).to("cuda")
    torch.cuda.synchronize()
    same(ix.search_device(qt, c.ef, c.k), one16, "device queries")
    same(ix.search_device(qt[5:8].contiguous(), c.ef, c.k), one3,
         "device queries, nq 3")
    ix.close()


def test_eval_accounting(index_of):
    """scan_rows counts the rows whose distance the beam evaluated (the
    README's HNSW bytes figure derives from it): every node of the chain but
    the entry, every leaf of the star."""
    c = hc.BY_NAME["chain-200-ef1"]
    ix = index_of(c)
    ix.perf_reset()
    ix.search(hc.queries(c)[:1], c.ef, c.k)
    p = ix.perf()
    assert p["scan_rows"] == 199 and p["scan_launches"] == 1, p
    assert p["scan_bytes"] == 199 * 8 * 4, p
    c = hc.BY_NAME["star-300-ef8"]
    ix = index_of(c)
    ix.perf_reset()
    ix.search(hc.queries(c)[:1], c.ef, c.k)
    p = ix.perf()
    assert p["scan_rows"] == 300 and p["scan_launches"] == 1, p


def test_errors_leave_the_handle_usable(index_of):
    from matrixone_amd.engine import MoannError
    c = hc.BY_NAME["deg-conn40"]
    ix = index_of(c)
    qs = hc.queries(c)
    with pytest.raises(MoannError, match="ef > 1024"):
        ix.search(qs, 1025, 10)
    with pytest.raises(MoannError, match="ef > 1024"):
        ix.search(qs, 64, 1025)         # ef is lifted to k
    with pytest.raises(MoannError, match="ef > 1024"):
        ix.search_filtered(qs, 1025, 10,
                           hc.slot_bitset(np.ones(len(hc.graph(c).levels),
                                                  dtype=bool)))
    with pytest.raises(MoannError, match="dim mismatch"):
        ix.search(np.zeros((2, hc.graph(c).dim + 1), dtype=np.float32),
                  c.ef, c.k)
    hc.check(c, *ix.search(qs, c.ef, c.k), *hc.reference(c))


# --------------------------------------------------------------- host layer

def test_host_l2_transform_keeps_padding():
    """vector_l2_ops + l2_distance: sqrt of the raw l2sq on valid slots;
    padding stays (-1, FLT_MAX)."""
    from matrixone_amd.hnsw import HnswSearch
    from matrixone_amd.ivfflat import RuntimeConfig
    c = hc.BY_NAME["pair-k-gt-n"]
    hs = HnswSearch(hc.graph_data(hc.graph(c)), op_type="vector_l2_ops",
                    ef_search=c.ef)
    hs.Load()
    ids, d64 = hs.Search(None, hc.queries(c),
                         RuntimeConfig(limit=c.k,
                                       orig_func_name="l2_distance"))
    hs.Destroy()
    ref_ids, ref_d = hc.reference(c)
    np.testing.assert_array_equal(ids, ref_ids)
    valid = ref_ids >= 0
    assert valid.sum() == 2 * len(ref_ids) and (~valid).any()
    assert d64.dtype == np.float64
    np.testing.assert_array_equal(d64[valid],
                                  np.sqrt(ref_d[valid].astype(np.float64)))
    np.testing.assert_array_equal(d64[~valid], np.float64(hc.FLT_MAX))


def test_multi_model_merge_with_a_model_smaller_than_k():
    from matrixone_amd.hnsw import MultiModelHnswSearch
    from matrixone_amd.ivfflat import RuntimeConfig
    from oracle import oracle as orc
    small, big, qs = hc.multi_models()
    k, ef = 10, 48
    mm = MultiModelHnswSearch([hc.graph_data(small), hc.graph_data(big)],
                              op_type="vector_l2sq_ops", ef_search=ef)
    mm.Load()
    ids, d64 = mm.Search(None, qs, RuntimeConfig(
        limit=k, orig_func_name="l2_distance_sq"))
    mm.Destroy()
    per = [[H.oracle_search(g, q, ef, k) for q in qs] for g in (small, big)]
    bi = np.stack([np.stack([r[0] for r in m]) for m in per])
    bd = np.stack([np.stack([r[1] for r in m]) for m in per])
    assert ((bi[0] >= 0).sum(1) == 3).all()
    mi, md = orc.topk_merge(bi, bd.astype(np.float32), k)
    assert (mi[0] >= 9_000_000).sum() == 3      # the small model is in play
    merged = hc.Case("multi-model", "host", ("multi",), ef, k, False,
                     nq=len(qs))
    hc.check(merged, ids, d64.astype(np.float32), mi, md)
    for row in ids:
        live = np.flatnonzero(row >= 0)
        assert live.size == k and (live == np.arange(live.size)).all(), row
