"""Case table shared by tests/test_refine_ref.py (CPU self-test of the
two-stage reference) and tests/test_refine_gpu.py (the HIP refine path
against that reference). Inputs are seeded and tiny; every reference is
computed once per process and shared."""

from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import oracle as orc
from oracle import refine as rf

# explicit list sizes: an empty list, a single row, 64 +- 1, an odd group
# count (3 groups: the scan's second-group-absent path), and lists spanning
# two (577 rows = 10 groups) and three (1100 rows = 18 groups) 8-group chunks
SIZES = (0, 1, 63, 64, 65, 129, 200, 577, 1100)
NLIST = len(SIZES)
ID_OFFSET = 1000

METRICS = {
    "l2sq": (orc.METRIC_L2SQ, False),
    "l2": (orc.METRIC_L2, True),
    "ip": (orc.METRIC_IP, False),
    "cos": (orc.METRIC_COS, False),
    "l1": (orc.METRIC_L1, False),
}

# mixed-width launch: queries per list under the one-hot centroids, probe=1
ONEHOT_COUNTS = {1: 17, 2: 8, 3: 9, 5: 16, 7: 1, 8: 40}
FLOOD_ROWS = 1500


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@dataclass(frozen=True)
class Corpus:
    vecs: np.ndarray
    cents: np.ndarray
    assign: np.ndarray
    ids: np.ndarray
    idx: orc.IvfIndex
    params: tuple
    codes: np.ndarray


@lru_cache(maxsize=None)
def corpus(kind: str, d: int) -> Corpus:
    rng = np.random.Generator(np.random.PCG64(_seed("corpus", kind, d)))
    sizes = list(SIZES)
    if kind == "dup4":
        sizes[-1] += 1          # 2200 rows = 550 vectors x 4
    elif kind == "flood":
        sizes[-1] = 1600
    n = sum(sizes)
    vecs = rng.standard_normal((n, d), dtype=np.float32)
    cents = rng.standard_normal((NLIST, d), dtype=np.float32)
    assign = rng.permutation(np.repeat(np.arange(NLIST), sizes))
    if kind == "dup4":
        vecs = np.repeat(vecs[:n // 4], 4, axis=0)[rng.permutation(n)]
    elif kind == "flood":
        # 1500 identical rows in the last list
        last = np.flatnonzero(assign == NLIST - 1)[:FLOOD_ROWS]
        vecs[last] = vecs[last[0]]
    elif kind == "onehot":
        cents = np.zeros((NLIST, d), dtype=np.float32)
        cents[np.arange(NLIST), np.arange(NLIST)] = 8.0
    vecs = np.ascontiguousarray(vecs)
    ids = rng.permutation(n).astype(np.int64) + ID_OFFSET
    idx = orc.IvfIndex(cents, vecs, assign, ids=ids)
    params = rf.rq_params(vecs)
    codes = rf.rq_quantize(vecs, *params)
    return Corpus(vecs, cents, assign, ids, idx, params, codes)


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    metric: str
    nq: int
    k: int = 10
    depth: int = 32
    kind: str = "std"           # corpus kind
    probe: int = NLIST
    qseed: int = 0
    filt: str = ""              # "", "rate30", "lists", "del_top1"

    @property
    def R(self):
        return max(self.k, self.depth)


def queries(c: Case) -> np.ndarray:
    return _queries(c.kind, c.d, c.nq, c.qseed)


@lru_cache(maxsize=None)
def _queries(kind, d, nq, qseed):
    rng = np.random.Generator(np.random.PCG64(_seed("q", d, qseed)))
    if kind == "onehot":
        cp = corpus(kind, d)
        lists = np.repeat(list(ONEHOT_COUNTS), list(ONEHOT_COUNTS.values()))
        assert lists.size == nq
        lists = rng.permutation(lists)
        return (cp.cents[lists] + np.float32(0.1) *
                rng.standard_normal((nq, d), dtype=np.float32))
    q = rng.standard_normal((nq, d), dtype=np.float32)
    if kind == "flood":
        # every other query sits next to the 1500 identical rows, so they
        # all tie on byte distance at the top-R boundary
        cp = corpus(kind, d)
        v = cp.vecs[np.flatnonzero(cp.assign == NLIST - 1)[0]]
        q[::2] = v + np.float32(0.3) * q[::2]
    return np.ascontiguousarray(q)


def reference(c: Case) -> rf.TwoStageRef:
    return _reference(c.kind, c.d, c.metric, c.nq, c.qseed, c.probe)


@lru_cache(maxsize=None)
def _reference(kind, d, metric, nq, qseed, probe):
    cp = corpus(kind, d)
    om, orig_l2 = METRICS[metric]
    return rf.build_ref(cp.idx, om, _queries(kind, d, nq, qseed), probe,
                        orig_l2=orig_l2, params=cp.params, codes=cp.codes)


def mask_without_ids(c: Case, ids) -> np.ndarray:
    """Row mask with the rows of `ids` cleared (soft delete)."""
    cp = corpus(c.kind, c.d)
    return ~np.isin(cp.ids, np.asarray(ids).ravel())


def allowed_rows(c: Case):
    """Bool mask over rows for filtered / deleted cases, else None."""
    if not c.filt:
        return None
    cp = corpus(c.kind, c.d)
    n = cp.vecs.shape[0]
    rng = np.random.Generator(np.random.PCG64(_seed("filt", c.name)))
    if c.filt == "rate30":
        return rng.random(n) < 0.3
    if c.filt == "lists":
        # per-list pass counts: none / fewer than k / fewer than R / half / all
        keep = {1: 0, 2: 5, 3: 20, 5: None, 7: 0.5, 8: 0.5}
        m = np.zeros(n, dtype=bool)
        for l, spec in keep.items():
            rows = np.flatnonzero(cp.assign == l)
            if spec is None:
                m[rows] = True
            elif isinstance(spec, float):
                m[rows] = rng.random(rows.size) < spec
            else:
                m[rng.choice(rows, spec, replace=False)] = True
        return m
    if c.filt == "del_top1":
        first, _ = rf.ideal_two_stage(reference(c), c.k, c.R)
        return mask_without_ids(c, first[:, 0])
    raise ValueError(c.filt)


def _table():
    t = []
    # tile geometry: every non-empty list sees all nq queries
    for d in (768, 64):
        for nq in (1, 8, 9, 16, 17, 25, 33):
            t.append(Case(f"tile-d{d}-nq{nq}", d, "l2sq", nq))
    t.append(Case("tile-mixed", 64, "l2sq", sum(ONEHOT_COUNTS.values()),
                  kind="onehot", probe=1))
    # metrics x dims, full depth (== exact search) and depth 32
    for metric in METRICS:
        for d in (16, 48, 64, 100, 67, 768):
            for depth in (4096, 32):
                t.append(Case(f"md-{metric}-d{d}-R{depth}", d, metric, 25,
                              depth=depth))
    # last QT=16 dot size and the first size past it
    for d in (3056, 3072):
        for metric in ("l2sq", "ip"):
            for depth in (4096, 32):
                t.append(Case(f"big-{metric}-d{d}-R{depth}", d, metric, 17,
                              depth=depth))
    # R and k
    t.append(Case("rk-k50-depth8", 64, "l2sq", 25, k=50, depth=8))
    t.append(Case("rk-k1", 64, "l2sq", 25, k=1))
    t.append(Case("rk-depth10", 64, "l2sq", 25, depth=10))
    t.append(Case("rk-k200-depth4096", 64, "l2sq", 25, k=200, depth=4096))
    t.append(Case("rk-reenable-depth16", 64, "l2sq", 25, depth=16))
    # filter and delete
    t.append(Case("filt-rate30", 64, "l2sq", 25, filt="rate30"))
    t.append(Case("filt-lists", 64, "l2sq", sum(ONEHOT_COUNTS.values()),
                  kind="onehot", probe=1, filt="lists"))
    t.append(Case("delete-top1", 64, "l2sq", 25, filt="del_top1"))
    # ties
    t.append(Case("ties-dup4", 64, "l2sq", 25, k=12, kind="dup4"))
    t.append(Case("ties-flood", 64, "l2sq", 16, kind="flood"))
    # pipelined batches (the benchmark's submit/collect path, d=768)
    for i, nq in enumerate((33, 1, 16, 25, 33)):
        t.append(Case(f"pipe-b{i}-nq{nq}", 768, "l2sq", nq, qseed=100 + i))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the skip cap of check_two_stage: MUST candidates within the tolerance of
# the cut-off, over a whole case
SKIP_CAP = 0.01
