"""Case table shared by tests/test_hnsw_cases_ref.py (CPU self-test of the
cases, the oracle and a list restatement of the kernel) and
tests/test_hnsw_edges_gpu.py (the HIP beam kernel against the oracle on the
same graph). Graphs are seeded and small; every graph, query set and
reference is built once per process and shared.

Two kinds of case:

exact      hand-built graphs over small integer coordinates. Every l2sq / ip
           partial sum is an integer below 2^24, so f32 is exact in any
           summation order and the kernel must equal the oracle bit for bit,
           ids and distances. Tie handling at the radius differs between
           usearch's heaps and the kernel's sorted list, so each exact case
           either keeps everything it can reach (ef >= the level-0 component
           the beam starts in) or has pairwise-distinct query distances over
           that component; test_hnsw_cases_ref.py asserts it.
tolerance  graphs built by the reference engine over random rows, compared
           with the distance band tests/test_hnsw_gpu.py already uses; id
           differences are capped at EXCUSE_CAP of the positions.
"""

from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import hnsw as H

FLT_MAX = np.float32(np.finfo(np.float32).max)
METRIC_NAME = {H.METRIC_L2SQ: "l2sq", H.METRIC_IP: "ip", H.METRIC_COS: "cos"}

# the comparator band (tests/test_hnsw_gpu.py::test_hnsw_gpu_vs_oracle) and
# the share of positions whose id may differ inside it (the same test's
# allowance against usearch)
RTOL, ATOL = 2e-5, 5e-5
EXCUSE_CAP = 0.05


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _rng(*parts):
    return np.random.Generator(np.random.PCG64(_seed(*parts)))


def graph_data(g: H.HnswGraph):
    """oracle.hnsw.HnswGraph -> matrixone_amd.hnsw.HnswGraphData."""
    from matrixone_amd.hnsw import HnswGraphData
    return HnswGraphData(dim=g.dim, metric=METRIC_NAME[g.metric],
                         entry_slot=g.entry_slot, max_level=g.max_level,
                         levels=g.levels, keys=g.keys, vecs=g.vecs, adj=g.adj)


# ---------------------------------------------------------------- builders

def make_graph(dim, metric, vecs, levels, lists, entry, keys=None):
    """lists[lvl] maps slot -> neighbour slots in tape order."""
    n = len(vecs)
    levels = np.asarray(levels, dtype=np.int32)
    max_level = int(levels.max())
    adj = []
    for lvl in range(max_level + 1):
        per = lists[lvl] if lvl < len(lists) else {}
        offs = np.zeros(n + 1, dtype=np.int64)
        for s in range(n):
            offs[s + 1] = offs[s] + len(per.get(s, ()))
        nbrs = np.zeros(int(offs[-1]), dtype=np.uint32)
        for s, l in per.items():
            nbrs[offs[s]:offs[s + 1]] = l
        adj.append((offs, nbrs))
    if keys is None:
        keys = np.arange(n)
    v = np.zeros((n, dim), dtype=np.float32)
    v[:] = np.asarray(vecs, dtype=np.float32)
    return H.HnswGraph(dim, metric, int(entry), max_level, levels,
                       np.asarray(keys, dtype=np.uint64), v, adj)


def _band(order, width, rng):
    """Undirected band graph over `order` (each node linked to the `width`
    nodes on either side), neighbour lists shuffled."""
    per = {}
    m = len(order)
    for i, s in enumerate(order):
        l = [order[j] for j in range(max(0, i - width), min(m, i + width + 1))
             if j != i]
        per[s] = [int(x) for x in rng.permutation(l)]
    return per


@lru_cache(maxsize=None)
def chain_graph(n):
    vecs = np.zeros((n, 8), dtype=np.float32)
    vecs[:, 0] = np.arange(n)
    l0 = {i: [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)}
    return make_graph(8, H.METRIC_L2SQ, vecs, np.zeros(n), [l0], 0,
                      keys=np.arange(n) * 3 + 7)


@lru_cache(maxsize=None)
def single_graph():
    return make_graph(4, H.METRIC_L2SQ, [[3, 1, 0, 2]], [0], [{}], 0,
                      keys=[41])


@lru_cache(maxsize=None)
def pair_graph():
    return make_graph(4, H.METRIC_L2SQ, [[3, 1, 0, 2], [0, 5, 1, 1]], [0, 0],
                      [{0: [1], 1: [0]}], 1, keys=[41, 17])


@lru_cache(maxsize=None)
def isolated_graph():
    """n = 50; the entry's level-0 list is empty."""
    n, entry = 50, 23
    rng = _rng("isolated")
    vecs = np.zeros((n, 4), dtype=np.float32)
    vecs[:, 0] = rng.permutation(n)
    vecs[:, 1] = rng.integers(0, 5, n)
    others = [s for s in range(n) if s != entry]
    return make_graph(4, H.METRIC_L2SQ, vecs, np.zeros(n),
                      [_band(others, 2, rng)], entry)


@lru_cache(maxsize=None)
def two_component_graph():
    """25 nodes around the entry, 35 unreachable ones nearer the queries."""
    n = 60
    rng = _rng("twocomp")
    slots = [int(s) for s in rng.permutation(n)]
    a, b = slots[:25], slots[25:]
    vecs = np.zeros((n, 4), dtype=np.float32)
    vecs[a, 0] = 100 + rng.permutation(25)
    vecs[b, 0] = rng.permutation(35)
    vecs[:, 2] = rng.integers(0, 4, n)
    l0 = _band(a, 3, rng)
    l0.update(_band(b, 3, rng))
    return make_graph(4, H.METRIC_L2SQ, vecs, np.zeros(n), [l0], a[7])


@lru_cache(maxsize=None)
def star_graph(leaves):
    """One hub (the entry) listing every leaf; each leaf lists the hub. The
    leaf nearest query 0 is the LAST hub neighbour and the leaf nearest
    query 1 sits past position 1024 where the list is that long."""
    n, hub = leaves + 1, 17
    rng = _rng("star", leaves)
    leaf_slots = [s for s in range(n) if s != hub]
    x = rng.permutation(leaves) + 1                 # distinct 1..leaves
    vecs = np.zeros((n, 4), dtype=np.float32)
    vecs[leaf_slots, 0] = x
    vecs[leaf_slots, 1] = x % 3
    vecs[leaf_slots, 3] = 1
    order = [int(s) for s in rng.permutation(leaf_slots)]
    far = leaf_slots[int(np.argmax(x))]             # nearest to query 0
    near = leaf_slots[int(np.argmin(x))]            # nearest to query 1
    order.remove(far)
    order.remove(near)
    order.insert(len(order) - 40, near)
    order.append(far)
    l0 = {s: [hub] for s in leaf_slots}
    l0[hub] = order
    return make_graph(4, H.METRIC_L2SQ, vecs, np.zeros(n), [l0], hub,
                      keys=np.arange(n) * 5 + 11)


TOWER_Q = np.array([1, 2, 0, 0, 0, 0, 0, 3], dtype=np.float32)


@lru_cache(maxsize=None)
def tower_graph(metric):
    """max_level 3. Each node has an integer score s, its distance rank:
    l2sq distance s^2, ip distance 1 + s. `alt` nodes reach the same
    distance from other coordinates (the equal-distance decoys).

    level 3  the entry E alone, empty list.
    level 2  E lists F0..F39. The running minimum improves in each 16-wide
             round: F0, F3 (round 1), F20 (round 2), F37 (round 3, the
             overall minimum). F37 lists the decoy D (position 5, same
             distance as F37: no move), G (position 9, closer) and G2
             (position 12, same distance as G: the first one wins).
    level 1  G starts a 30-hop chain C1..C30 of strictly closer nodes.
    level 0  three components: A = {E, F*, D}, B = {G, C*, T*} and
             X = {G2, X*}. The correct search ends in B, where ef = 16
             meets 71 nodes with distinct distances. A descent that stops
             after the first 16 neighbours stays in A; one that takes the
             later of two equal minima lands in X."""
    rng = _rng("tower")          # same topology for both metrics
    names, score, alt, level = [], {}, set(), {}

    def node(name, s, lvl, is_alt=False):
        names.append(name)
        score[name], level[name] = s, lvl
        if is_alt:
            alt.add(name)

    node("E", 1000, 3)
    for j in range(40):
        node(f"F{j}", 850 + 3 * j, 2)
    score["F3"], score["F20"], score["F37"] = 800, 700, 600
    node("D", 600, 2, True)
    node("G", 550, 2)
    node("G2", 550, 2, True)
    for i in range(1, 31):
        node(f"C{i}", 550 - 10 * i, 1)
    for j in range(40):
        node(f"T{j}", 5 + 6 * j, 0)
    for j in range(12):
        node(f"X{j}", 400 + 7 * j, 0)
    slot = {nm: int(s) for nm, s in zip(names, rng.permutation(len(names)))}
    n = len(names)
    vecs = np.zeros((n, 8), dtype=np.float32)
    levels = np.zeros(n, dtype=np.int32)
    for nm in names:
        s = score[nm]
        if metric == H.METRIC_L2SQ:
            off = [0, s, 0, 0, 0, 0, 0, 0] if nm in alt else [s, 0, 0, 0, 0, 0, 0, 0]
            vecs[slot[nm]] = TOWER_Q + np.array(off, dtype=np.float32)
        else:
            vecs[slot[nm]] = ([-s + 2, -1, 9, 0, 4, 0, 0, 0] if nm in alt
                              else [-s, 0, 5, 0, 0, 7, 0, 0])
        levels[slot[nm]] = level[nm]

    def S(*ns):
        return [slot[x] for x in ns]

    fs = [f"F{j}" for j in range(40)]
    l2 = {slot["E"]: S(*fs)}
    for f in fs:
        l2[slot[f]] = S("E")
    l2[slot["F37"]] = S("E", "F36", "F38", "F1", "F2", "D", "F4", "F5", "F6",
                        "G", "F7", "F8", "G2", "F9")
    l2[slot["D"]] = S("F37")
    l2[slot["G"]] = S("F37")
    l2[slot["G2"]] = S("F37")
    cs = ["G"] + [f"C{i}" for i in range(1, 31)]
    l1 = {slot["G"]: S("F37", "C1"), slot["G2"]: S("F37"),
          slot["F37"]: S("G", "G2"), slot["E"]: S("F0"),
          slot["F0"]: S("E")}
    for i in range(1, 31):
        l1[slot[cs[i]]] = S(*([cs[i - 1]] + ([cs[i + 1]] if i < 30 else [])))

    def by_score(group):
        return [slot[x] for x in sorted(group, key=lambda x: (score[x], x))]

    l0 = _band(by_score(["E", "D"] + fs), 2, rng)
    l0.update(_band(by_score(cs + [f"T{j}" for j in range(40)]), 2, rng))
    l0.update(_band(by_score(["G2"] + [f"X{j}" for j in range(12)]), 2, rng))
    g = make_graph(8, metric, vecs, levels, [l0, l1, l2, {}], slot["E"],
                   keys=np.arange(n) + 500)
    g.names = slot
    return g


@lru_cache(maxsize=None)
def lattice_graph():
    """4x4x4x4 integer lattice, nodes linked within l2sq <= 2. The keys are
    a non-monotonic permutation of the slots (slot*7 mod 256, + 1000), so
    ordering ties by key instead of slot changes the output."""
    pts = np.stack(np.meshgrid(*[np.arange(4)] * 4, indexing="ij"),
                   -1).reshape(-1, 4)
    rng = _rng("lattice")
    pts = pts[rng.permutation(256)]
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    l0 = {}
    for s in range(256):
        nb = np.flatnonzero((d2[s] <= 2) & (np.arange(256) != s))
        l0[s] = [int(x) for x in rng.permutation(nb)]
    return make_graph(4, H.METRIC_L2SQ, pts, np.zeros(256), [l0], 0,
                      keys=(np.arange(256) * 7) % 256 + 1000)


@lru_cache(maxsize=None)
def multi_models():
    """(small, big, queries) for the multi-model merge: a hand-built model
    of 3 fully-linked nodes (fewer than k) next to query 0, and an engine-
    built model of 2500 rows."""
    d = 16
    big = random_graph(2500, d, H.METRIC_L2SQ, 16, "multi")
    q = _queries_near(big, 8, "multi")
    rng = _rng("small")
    vecs = q[0] + np.float32(0.2) * rng.standard_normal((3, d),
                                                         dtype=np.float32)
    l0 = {0: [1, 2], 1: [2, 0], 2: [0, 1]}
    small = make_graph(d, H.METRIC_L2SQ, vecs, np.zeros(3), [l0], 1,
                       keys=np.arange(3) + 9_000_000)
    return small, big, q


@lru_cache(maxsize=None)
def random_graph(n, d, metric, conn, tag):
    rng = _rng("rows", n, d, tag)
    vecs = rng.standard_normal((n, d), dtype=np.float32)
    if d < 4:
        # hundreds of rows on a line or a small sphere: spread them, or
        # their l2sq gaps fall inside the comparator band
        vecs *= np.float32(16)
    ix = H.RefHnsw(d, metric=metric, connectivity=conn, expansion_add=64,
                   expansion_search=48, capacity=n, threads=4)
    ix.add(vecs, keys=np.arange(n, dtype=np.uint64) * 3 + 100)
    return ix.export_graph()


def _queries_near(g, nq, tag):
    """Perturbed stored rows: pure random queries pack cosine distances too
    tightly for the comparator band."""
    rng = _rng("q", tag, g.dim, len(g.levels))
    rows = rng.choice(len(g.levels), nq, replace=False)
    noise = rng.standard_normal((nq, g.dim), dtype=np.float32)
    return np.ascontiguousarray(g.vecs[rows] + np.float32(0.5) * noise)


# ------------------------------------------------------------------- cases

@dataclass(frozen=True)
class Case:
    name: str
    group: str
    graph: tuple            # (builder name, *args)
    ef: int
    k: int
    exact: bool
    nq: int = 2
    filt: str = ""          # "", "third", "half", "none", "few", "entry", "tail"

    @property
    def filtered(self):
        return bool(self.filt)


_BUILDERS = {
    "chain": chain_graph, "single": single_graph, "pair": pair_graph,
    "isolated": isolated_graph, "twocomp": two_component_graph,
    "star": star_graph, "tower": tower_graph, "lattice": lattice_graph,
    "random": random_graph,
}


def graph(c: Case) -> H.HnswGraph:
    return _BUILDERS[c.graph[0]](*c.graph[1:])


def queries(c: Case) -> np.ndarray:
    return _queries(c.graph, c.nq, c.name if c.filt == "tail" else "")


@lru_cache(maxsize=None)
def _queries(gspec, nq, tag):
    g = _BUILDERS[gspec[0]](*gspec[1:])
    n, kind = len(g.levels), gspec[0]
    q = np.zeros((nq, g.dim), dtype=np.float32)
    if kind == "chain":
        q[:, 0] = [n - 1, n + 2][:nq]       # the far end, and past it
    elif kind in ("single", "pair"):
        q[:] = [[1, 0, 2, 2], [4, 4, 0, 1]][:nq]
    elif kind in ("isolated", "twocomp"):
        q[:] = [[-3, 1, 2, 0], [7, 0, 1, 1]][:nq]
    elif kind == "star":
        q[:] = [[n + 4, 1, 0, 0], [-4, 1, 0, 0]][:nq]
    elif kind == "tower":
        q[:] = TOWER_Q
    elif kind == "lattice":
        q[:] = [[1, 2, 0, 3], [0, 0, 0, 0], [5, 1, 2, -1], [2, 2, 2, 2]][:nq]
    else:
        q = _queries_near(g, nq, "near")
        if tag:
            # the last slot (the filter's last word holds one live bit)
            # must come back: aim query 0 at it
            q[0] = g.vecs[n - 1] + np.float32(0.05) * q[0]
    return np.ascontiguousarray(q)


def pass_slots(c: Case):
    """Bool mask over slots for filtered cases, else None."""
    if not c.filt:
        return None
    g = graph(c)
    n = len(g.levels)
    rng = _rng("filt", c.name)
    if c.filt == "third":
        return np.arange(n) % 3 == 0
    if c.filt == "none":
        return np.zeros(n, dtype=bool)
    if c.filt == "few":
        # the 3 rows nearest query 0: that query returns exactly them, the
        # others whatever of the three their beams come across
        m = np.zeros(n, dtype=bool)
        d = ((g.vecs - queries(c)[0]) ** 2).sum(1)
        m[np.argsort(d, kind="stable")[:3]] = True
        return m
    m = rng.random(n) < 0.5
    if c.filt == "entry":
        m[g.entry_slot] = False
    elif c.filt == "tail":
        m[n - 1] = True
    return m


def slot_bitset(mask) -> np.ndarray:
    n = len(mask)
    idx = np.flatnonzero(mask)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, idx // 32,
                     np.uint32(1) << (idx % 32).astype(np.uint32))
    return words


def reference(c: Case):
    """(ids, dists) of the oracle, [nq][k]."""
    ids, d = _reference(c)
    return ids[:, :c.k], d[:, :c.k]


def reference_plus_one(c: Case):
    """The oracle's output one rank deeper where ef allows (the same search:
    only the shrink to k differs)."""
    return _reference(c)


@lru_cache(maxsize=None)
def _reference(c: Case):
    g, qs = graph(c), queries(c)
    kk = c.k + 1 if c.ef > c.k else c.k
    ef = max(c.ef, c.k)
    out_i, out_d = [], []
    mask = pass_slots(c)
    if mask is not None:
        aset = set(int(x) for x in g.keys[mask])
    for q in qs:
        if mask is None:
            i, d = H.oracle_search(g, q, ef, kk)
        else:
            i, d = H.oracle_search_filtered_batch(g, q, ef, kk,
                                                  lambda key: key in aset)
        out_i.append(i)
        out_d.append(d)
    ids, d = np.stack(out_i), np.stack(out_d)
    ids.setflags(write=False)
    d.setflags(write=False)
    return ids, d


def _table():
    L2, IP, COS = H.METRIC_L2SQ, H.METRIC_IP, H.METRIC_COS
    t = [
        # a level-0 path longer than 16*ef + 64 expansions
        Case("chain-200-ef1", "chains", ("chain", 200), 1, 1, True),
        Case("chain-400-ef8", "chains", ("chain", 400), 8, 8, True),
        Case("chain-400-ef8-filt", "chains", ("chain", 400), 8, 8, True,
             filt="third"),
        Case("single-node", "degenerate", ("single",), 8, 5, True),
        Case("pair-k-gt-n", "degenerate", ("pair",), 8, 5, True),
        Case("entry-isolated", "degenerate", ("isolated",), 8, 5, True),
        Case("two-components", "degenerate", ("twocomp",), 32, 10, True),
        # sort widths 512 and 2048; more new keys than the list holds
        Case("star-300-ef8", "stars", ("star", 300), 8, 8, True),
        Case("star-300-ef1024", "stars", ("star", 300), 1024, 100, True),
        Case("star-1100-ef8", "stars", ("star", 1100), 8, 8, True),
        Case("star-1100-ef1024", "stars", ("star", 1100), 1024, 100, True),
        Case("tower-fan40-l2sq", "tower", ("tower", L2), 16, 10, True, nq=1),
        Case("tower-fan40-ip", "tower", ("tower", IP), 16, 10, True, nq=1),
        Case("ties-lattice", "ties", ("lattice",), 256, 256, True, nq=4),
        # row widths: 192 quads (3 lane iterations), 257 (a one-quad fifth
        # iteration), 65 (one lane takes a second iteration), 1 (one lane)
        Case("wide-768-l2sq", "wide", ("random", 1500, 768, L2, 16, "w"),
             64, 10, False, nq=16),
        Case("wide-768-cos", "wide", ("random", 1500, 768, COS, 16, "w"),
             64, 10, False, nq=16),
        Case("wide-1028-ip", "wide", ("random", 1500, 1028, IP, 16, "w"),
             64, 10, False, nq=8),
        Case("wide-260-cos", "wide", ("random", 1200, 260, COS, 16, "w"),
             64, 10, False, nq=16),
        Case("tiny-d1", "tiny", ("random", 500, 1, L2, 16, "t"), 32, 10,
             False, nq=8),
        Case("tiny-d3", "tiny", ("random", 500, 3, COS, 16, "t"), 32, 10,
             False, nq=8),
        # level-0 degree above 64: sort width 128
        Case("deg-conn40", "degree", ("random", 2000, 16, L2, 40, "deg"),
             64, 10, False, nq=8),
        # list above 1024 entries: two entries per thread in the radius scan
        Case("filt-ef600", "filtered", ("random", 3000, 24, L2, 16, "f"),
             600, 20, False, nq=4, filt="half"),
        Case("filt-none", "filtered", ("random", 3000, 24, L2, 16, "f"),
             48, 10, False, nq=8, filt="none"),
        Case("filt-few", "filtered", ("random", 3000, 24, L2, 16, "f"),
             48, 10, False, nq=8, filt="few"),
        Case("filt-entry-fails", "filtered",
             ("random", 3000, 24, L2, 16, "f"), 48, 10, False, nq=8,
             filt="entry"),
        Case("filt-tailbits", "filtered", ("random", 3001, 24, L2, 16, "f"),
             48, 10, False, nq=8, filt="tail"),
    ]
    return t


# the case whose handle the workspace-reuse sequence runs on
REUSE_CASE = "wide-768-l2sq"

CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = sorted({c.group for c in CASES})


def names(group=None, **kw):
    return [c.name for c in CASES
            if (group is None or c.group == group)
            and all(getattr(c, a) == v for a, v in kw.items())]


# -------------------------------------------------------------- comparator

def band(ref_d):
    return ATOL + RTOL * np.abs(np.asarray(ref_d, dtype=np.float64))


def check(c: Case, ids, dists, ref_ids, ref_dists) -> int:
    """Compare a result with the reference of case `c`; returns the number
    of excused positions (ids that differ inside the distance band).

    exact cases      ids and distances equal, tolerance 0.
    tolerance cases  distances within rtol=2e-5, atol=5e-5 of the reference
                     at every position; an id may differ only where the
                     distance there is inside that band, at no more than
                     EXCUSE_CAP of the nq*k positions."""
    ids, dists = np.asarray(ids), np.asarray(dists)
    assert ids.shape == ref_ids.shape and dists.shape == ref_dists.shape, (
        c.name, ids.shape, ref_ids.shape)
    if c.exact:
        np.testing.assert_array_equal(ids, ref_ids, err_msg=f"{c.name}: ids")
        np.testing.assert_array_equal(dists, ref_dists,
                                      err_msg=f"{c.name}: dists")
        return 0
    np.testing.assert_allclose(dists, ref_dists, rtol=RTOL, atol=ATOL,
                               err_msg=f"{c.name}: dists")
    diff = ids != ref_ids
    gap = np.abs(dists.astype(np.float64) - ref_dists.astype(np.float64))
    bad = diff & ~(gap <= band(ref_dists))
    assert not bad.any(), (c.name, np.argwhere(bad)[:4].tolist())
    excused = int(diff.sum())
    assert excused <= EXCUSE_CAP * ids.size, (
        f"{c.name}: {excused} of {ids.size} ids differ inside the band")
    return excused


# ------------------------------------------- helpers the ref tests share

def level0_component(g: H.HnswGraph, start: int) -> np.ndarray:
    """Slots reachable from `start` over level-0 lists."""
    seen, todo = {int(start)}, [int(start)]
    while todo:
        s = todo.pop()
        for nb in g.neighbors(s, 0):
            if int(nb) not in seen:
                seen.add(int(nb))
                todo.append(int(nb))
    return np.array(sorted(seen), dtype=np.int64)


def descend(g: H.HnswGraph, q, dist=None, fan=None):
    """Greedy descent to the level-0 start: per scan, the FIRST strict
    minimum of the list (what usearch's running update ends on). `fan`
    limits the scan to the first `fan` neighbours (a corruption)."""
    if dist is None:
        def dist(s):
            return float(H._usearch_dist(g.metric, g.vecs[s], q))
    cur = g.entry_slot
    cur_d = dist(cur)
    for level in range(g.max_level, 0, -1):
        while True:
            best, bs = cur_d, -1
            for nb in g.neighbors(cur, level)[:fan]:
                d = dist(int(nb))
                if d < best:
                    best, bs = d, int(nb)
            if bs < 0:
                break
            cur, cur_d = bs, best
    return cur, cur_d
