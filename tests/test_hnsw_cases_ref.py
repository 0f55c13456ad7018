"""CPU self-test of the HNSW case table (tests/hnsw_cases.py): the graphs
are ones usearch could emit, the exact cases cannot hit the one place where
the kernel and the oracle may legitimately differ (ties at the radius), the
oracle equals a brute-force answer where the search is exhaustive, the
comparator's excuse cap cannot be used up by near-ties, and a list
restatement of the kernel passes the comparator on every unfiltered case
while each seeded corruption of it is rejected by the case that owns it —
so the GPU tests cannot pass vacuously."""

import numpy as np
import pytest

import hnsw_cases as hc
from oracle import hnsw as H


def _dist_fn(g, q, dims=None):
    def dist(s):
        return float(H._usearch_dist(g.metric, g.vecs[s][:dims], q[:dims]))
    return dist


def list_model(g, q, ef, k, *, dist=None, cap=None, fan=None, l0cap=None,
               visited=None, by_key=False):
    """The unfiltered kernel restated over a Python list: the candidates
    sorted by (dist, slot), expand the first unexpanded entry, merge its
    unvisited neighbours, truncate at ef. The keyword arguments are the
    corruptions (all off by default)."""
    dist = dist or _dist_fn(g, q)
    cur, cur_d = hc.descend(g, q, dist=dist, fan=fan)
    visited = set() if visited is None else visited
    visited.add(cur)
    lst = [(cur_d, cur, False)]
    it = 0
    while cap is None or it < cap:
        bi = next((i for i, t in enumerate(lst) if not t[2]), None)
        if bi is None:
            break
        lst[bi] = (lst[bi][0], lst[bi][1], True)
        new = []
        for nb in g.neighbors(lst[bi][1], 0)[:l0cap]:
            if int(nb) not in visited:
                visited.add(int(nb))
                new.append((dist(int(nb)), int(nb), False))
        lst = sorted(lst + new, key=lambda t: t[:2])[:ef]
        it += 1
    out = [(d, s) for d, s, _ in lst[:k]]
    if by_key:
        out.sort(key=lambda t: (t[0], int(g.keys[t[1]])))
    ids = np.full(k, -1, dtype=np.int64)
    dists = np.full(k, hc.FLT_MAX, dtype=np.float32)
    for i, (d, s) in enumerate(out):
        ids[i], dists[i] = g.keys[s], d
    return ids, dists


def _model_batch(c, **kw):
    g, qs = hc.graph(c), hc.queries(c)
    ef = max(c.ef, c.k)
    per_q = kw.pop("per_q", None)
    res = [list_model(g, q, ef, c.k, **(per_q(g, q) if per_q else {}), **kw)
           for q in qs]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _rejected(c, ids, d):
    with pytest.raises(AssertionError):
        hc.check(c, ids, d, *hc.reference(c))


# ------------------------------------------------------------ case sanity

@pytest.mark.parametrize("name", [c.name for c in hc.CASES])
def test_graph_is_one_usearch_could_emit(name):
    g = hc.graph(hc.BY_NAME[name])
    n = len(g.levels)
    assert g.vecs.shape == (n, g.dim) and g.keys.shape == (n,)
    assert len(set(g.keys.tolist())) == n
    assert len(g.adj) == g.max_level + 1 == int(g.levels.max()) + 1
    assert g.levels[g.entry_slot] == g.max_level
    for lvl, (offs, nbrs) in enumerate(g.adj):
        assert offs[0] == 0 and offs[-1] == nbrs.size
        cnt = np.diff(offs)
        assert (cnt >= 0).all()
        assert not cnt[g.levels < lvl].any(), f"level {lvl}: list below level"
        if not nbrs.size:
            continue
        assert nbrs.max() < n
        assert (g.levels[nbrs] >= lvl).all(), f"level {lvl}: low neighbour"
        owner = np.repeat(np.arange(n), cnt)
        assert (owner != nbrs).all(), f"level {lvl}: self-loop"
        pairs = owner.astype(np.int64) * n + nbrs
        assert np.unique(pairs).size == pairs.size, f"level {lvl}: duplicate"


@pytest.mark.parametrize("name", hc.names(exact=True))
def test_exact_case_is_exact_and_tie_free(name):
    c = hc.BY_NAME[name]
    g, qs = hc.graph(c), hc.queries(c)
    v, q = g.vecs.astype(np.float64), qs.astype(np.float64)
    assert (v == np.rint(v)).all() and (q == np.rint(q)).all()
    # every partial sum of either metric is an integer below 2^24
    # (sums of non-negative terms: the total bounds every partial sum)
    for b in q:
        assert (((v - b) ** 2).sum(1) < 2 ** 24).all()
        assert (np.abs(v * b).sum(1) < 2 ** 24).all()
    ef = max(c.ef, c.k)
    for qi in range(len(qs)):
        start, _ = hc.descend(g, qs[qi])
        comp = hc.level0_component(g, start)
        d = np.array([H._usearch_dist(g.metric, g.vecs[s], qs[qi])
                      for s in comp])
        assert ef >= comp.size or np.unique(d).size == d.size, (
            f"{name} q{qi}: ties among {comp.size} reachable nodes, ef {ef}")


def test_case_preconditions():
    """The graph properties the cases are in the table for."""
    def maxdeg(g):
        return int(np.diff(g.adj[0][0]).max())
    assert maxdeg(hc.star_graph(300)) == 300            # sort width 512
    assert maxdeg(hc.star_graph(1100)) == 1100 > 1024   # second stride
    deg = maxdeg(hc.graph(hc.BY_NAME["deg-conn40"]))
    assert 64 < deg <= 128, deg                         # sort width 128
    for n, ef in ((200, 1), (400, 8)):
        assert n - 1 > 16 * ef + 64      # a path longer than the old bound
    assert 400 - 1 > 16 * (2 * 8) + 64   # ... and than the filtered one
    for m in (H.METRIC_L2SQ, H.METRIC_IP):
        g = hc.tower_graph(m)
        assert g.max_level == 3
        assert g.neighbors(g.entry_slot, 3).size == 0
        fan = g.neighbors(g.entry_slot, 2)
        assert fan.size == 40
        d = [H._usearch_dist(m, g.vecs[s], hc.TOWER_Q) for s in fan]
        assert int(np.argmin(d)) == 37 and sorted(d)[0] < sorted(d)[1]
        f37 = g.neighbors(int(fan[37]), 2)
        assert H._usearch_dist(m, g.vecs[f37[5]], hc.TOWER_Q) == d[37]
        assert (H._usearch_dist(m, g.vecs[f37[9]], hc.TOWER_Q) ==
                H._usearch_dist(m, g.vecs[f37[12]], hc.TOWER_Q) < d[37])
    c = hc.BY_NAME["filt-tailbits"]
    n = len(hc.graph(c).levels)
    assert n % 32 and hc.pass_slots(c)[n - 1]
    assert int(hc.graph(c).keys[n - 1]) in hc.reference(c)[0][0]
    c = hc.BY_NAME["filt-entry-fails"]
    assert not hc.pass_slots(c)[hc.graph(c).entry_slot]
    assert hc.pass_slots(hc.BY_NAME["filt-few"]).sum() == 3
    keys = hc.lattice_graph().keys.astype(np.int64)
    assert (np.diff(keys) < 0).any()     # key order is not slot order


# --------------------------------------------- the oracle on its own feet

EXHAUSTIVE = ["single-node", "pair-k-gt-n", "entry-isolated",
              "two-components", "star-300-ef1024", "ties-lattice"]


@pytest.mark.parametrize("name", EXHAUSTIVE)
def test_oracle_equals_bruteforce_over_component(name):
    """ef >= the reachable component: the oracle returns its exact top-k
    (f64 brute force), ordered by (dist, slot), then padding."""
    c = hc.BY_NAME[name]
    g, qs = hc.graph(c), hc.queries(c)
    ref_ids, ref_d = hc.reference(c)
    for qi in range(len(qs)):
        comp = hc.level0_component(g, hc.descend(g, qs[qi])[0])
        assert max(c.ef, c.k) >= comp.size
        a, b = g.vecs[comp].astype(np.float64), qs[qi].astype(np.float64)
        d = (((a - b) ** 2).sum(1) if g.metric == H.METRIC_L2SQ
             else 1.0 - a @ b)
        order = np.lexsort((comp, d))[:c.k]
        m = order.size
        np.testing.assert_array_equal(ref_ids[qi, :m],
                                      g.keys[comp[order]].astype(np.int64))
        np.testing.assert_array_equal(ref_d[qi, :m].astype(np.float64),
                                      d[order])
        assert (ref_ids[qi, m:] == -1).all()
        assert (ref_d[qi, m:] == hc.FLT_MAX).all()


def test_exhaustive_list_is_complete():
    for c in hc.CASES:
        if c.filtered or not c.exact or c.name in EXHAUSTIVE:
            continue
        g, qs = hc.graph(c), hc.queries(c)
        sizes = [hc.level0_component(g, hc.descend(g, q)[0]).size
                 for q in qs]
        assert max(c.ef, c.k) < max(sizes), c.name


@pytest.mark.parametrize("name", hc.names(exact=False))
def test_near_tie_budget(name):
    """Positions whose gap to the next reference distance lies inside the
    comparator band could swap ids legitimately; there must be too few of
    them to use up the excuse cap."""
    c = hc.BY_NAME[name]
    ids, d = hc.reference_plus_one(c)
    d = d.astype(np.float64)
    if d.shape[1] == c.k:                   # ef == k: no deeper rank
        d = np.concatenate([d, np.full((len(d), 1), np.inf)], 1)
    live = (ids[:, :c.k] >= 0) & (d[:, 1:c.k + 1] < float(hc.FLT_MAX))
    near = live & (d[:, 1:c.k + 1] - d[:, :c.k] <= hc.band(d[:, :c.k]))
    assert near.sum() <= hc.EXCUSE_CAP * ids.shape[0] * c.k, int(near.sum())


def test_reference_is_not_empty():
    """Every case but filt-none returns ids; filt-few returns its 3."""
    for c in hc.CASES:
        ids, _ = hc.reference(c)
        if c.name == "filt-none":
            assert (ids == -1).all()
        elif c.name == "filt-few":
            assert ((ids >= 0).sum(1) <= 3).all() and (ids[0] >= 0).sum() == 3
        else:
            assert (ids[:, 0] >= 0).all(), c.name


# ------------------------------------------------------------- list model

@pytest.mark.parametrize("name", hc.names(filt=""))
def test_list_model_matches_oracle(name):
    """The sorted-list formulation equals usearch's next/top heap pair."""
    c = hc.BY_NAME[name]
    hc.check(c, *_model_batch(c), *hc.reference(c))


@pytest.mark.parametrize("name", ["chain-200-ef1", "chain-400-ef8"])
def test_rejects_capped_expansions(name):
    c = hc.BY_NAME[name]
    _rejected(c, *_model_batch(c, cap=16 * c.ef + 64))


@pytest.mark.parametrize("name,dims", [("wide-768-l2sq", 256),
                                       ("wide-768-cos", 256),
                                       ("wide-260-cos", 256),
                                       ("wide-1028-ip", 1024)])
def test_rejects_short_distance(name, dims):
    """The first 64 quads only (a lane loop without its stride), and a row
    without its last quad (a dropped tail)."""
    c = hc.BY_NAME[name]
    _rejected(c, *_model_batch(
        c, per_q=lambda g, q: {"dist": _dist_fn(g, q, dims)}))


@pytest.mark.parametrize("name", ["tower-fan40-l2sq", "tower-fan40-ip"])
def test_rejects_one_round_descent(name):
    c = hc.BY_NAME[name]
    _rejected(c, *_model_batch(c, fan=16))


@pytest.mark.parametrize("name", ["star-1100-ef8", "star-1100-ef1024"])
def test_rejects_truncated_hub(name):
    c = hc.BY_NAME[name]
    _rejected(c, *_model_batch(c, l0cap=1024))


def test_rejects_stale_visited_set():
    """The workspace-reuse sequence: a query that starts from the previous
    query's visited set."""
    c = hc.BY_NAME[hc.REUSE_CASE]
    shared = set()
    _rejected(c, *_model_batch(c, visited=shared))


def test_rejects_tie_order_by_key():
    c = hc.BY_NAME["ties-lattice"]
    _rejected(c, *_model_batch(c, by_key=True))
