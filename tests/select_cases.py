"""Case table shared by tests/test_select_ref.py (CPU self-test of the
reference and of the cases' own conditions) and tests/test_select_gpu.py (the
radix and threshold-filter selection kernels against it, through
moann_select_topk). Inputs are seeded and small; every case and reference is
computed once per process and left unchanged.

The reference is the definition: sort (f2u(d) << 32) | index, take k, pad with
(-1, FLT_MAX). The radix select returns the same unless it ends in its
level-3 tie mode, which needs more than its 1024-key sort buffer of equal
values at the cut; no case holds a value more than MAX_REPEAT times in a row,
so both modes must equal the reference exactly.

The filter's rule (sample positions, threshold rank, capacity) is read from
the library (engine.select_plan), never restated here; `simulate` applies it
to a row on the CPU and says whether the filter must fall back."""

from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

FLT_MAX = np.finfo(np.float32).max
MAX_REPEAT = 256


def plan(count: int, k: int) -> dict:
    from matrixone_amd import engine
    return engine.select_plan(int(count), int(k))


@lru_cache(maxsize=None)
def constants() -> dict:
    p = plan(0, 1)
    return {"MIN": p["min_count"], "KMAX": p["kmax"], "CAP": p["capacity"]}


def f2u(d: np.ndarray) -> np.ndarray:
    """The kernels' monotone f32 -> u32 key."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    neg = (u >> 31).astype(bool)
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sample_positions(count: int, k: int) -> np.ndarray:
    from matrixone_amd import engine
    return engine.select_sample_positions(int(count), int(k))


@dataclass(frozen=True)
class Case:
    name: str
    k: int
    dists: np.ndarray   # all rows, concatenated
    qoffs: np.ndarray   # [nq + 1] int64

    @property
    def nq(self):
        return self.qoffs.size - 1

    def row(self, q):
        return self.dists[self.qoffs[q]:self.qoffs[q + 1]]


def _rng(*parts):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(parts).encode())))


def _case(name, k, rows):
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    qoffs = np.zeros(len(rows) + 1, dtype=np.int64)
    qoffs[1:] = np.cumsum([r.size for r in rows])
    d = np.concatenate(rows) if rows else np.zeros(0, np.float32)
    d.setflags(write=False)
    qoffs.setflags(write=False)
    return Case(name, k, d, qoffs)


def ragged_counts():
    """An odd first row, then the engage count and its neighbours: every
    off % 4 and every tail length occurs among the filtered rows."""
    M = constants()["MIN"]
    return [1001, M - 1, M, M + 1, M + 2, M + 3, M + 17, 3 * M + 5]


def _ragged(tag, k):
    rng = _rng("ragged")
    return _case(f"ragged-k{tag}", k,
                 [rng.standard_normal(n, dtype=np.float32)
                  for n in ragged_counts()])


def _short(k=64):
    rng = _rng("short")
    M = constants()["MIN"]
    return _case("short", k, [rng.standard_normal(n, dtype=np.float32)
                              for n in (0, 1, k - 1, k, k + 1, 0, M + 5, 0)])


def _special(k=64):
    """Negatives, both zeros and a block of FLT_MAX in a filtered row whose
    top k holds 5 negatives, 20 x -0.0, 20 x +0.0 and 19 positives; and a
    short row with fewer than k finite values."""
    rng = _rng("special")
    M = constants()["MIN"]
    a = np.abs(rng.standard_normal(M + 3617, dtype=np.float32)) + np.float32(1e-3)
    pos = rng.permutation(a.size)
    a[pos[:5]] = -np.abs(rng.standard_normal(5, dtype=np.float32)) - 1
    a[pos[5:25]] = np.float32(-0.0)
    a[pos[25:45]] = np.float32(0.0)
    a[7000:7200] = FLT_MAX
    b = rng.standard_normal(200, dtype=np.float32)
    b[rng.permutation(200)[:170]] = FLT_MAX     # 30 finite < k
    return _case("special", k, [np.float32([3, -1, 2]), a, b])


def _steered(name, k, count, smallest):
    """A row whose sampled positions hold its t smallest values (nothing else
    is that small: the filter collects t < k keys), or its largest values
    (the threshold passes nearly the whole row: overflow)."""
    rng = _rng(name)
    p = plan(count, k)
    assert p["filter"]
    sp = sample_positions(count, k)
    assert sp.size == p["sample"] and np.unique(sp).size == sp.size
    row = rng.standard_normal(count, dtype=np.float32)
    if smallest:
        assert p["rank"] < k
        row[sp[rng.permutation(sp.size)[:p["rank"]]]] = \
            np.float32(-50) - rng.random(p["rank"], dtype=np.float32)
    else:
        row[sp] = np.float32(50) + rng.random(sp.size, dtype=np.float32)
    lead = rng.standard_normal(3, dtype=np.float32)  # off % 4 == 3
    return _case(name, k, [lead, row])


@lru_cache(maxsize=None)
def cases():
    c = constants()
    M = c["MIN"]
    t = [_ragged(tag, k) for tag, k in (
        (1, 1), (10, 10), (64, 64), ("max", c["KMAX"]),
        ("max+1", c["KMAX"] + 1))]
    t.append(_short())
    t.append(_special())
    t.append(_steered("undershoot", 64, 3 * M, smallest=True))
    t.append(_steered("overflow", 64, 3 * M, smallest=False))
    t.append(_case("gauss20000", 64,
                   [_rng("gauss").standard_normal(20000, dtype=np.float32)]))
    return {x.name: x for x in t}


# static: the library (which knows the filter's largest k, "max") is loaded
# when a test runs, never while tests are collected
NAMES = ("ragged-k1", "ragged-k10", "ragged-k64", "ragged-kmax",
         "ragged-kmax+1", "short", "special", "undershoot", "overflow",
         "gauss20000")


def names():
    return list(NAMES)


@lru_cache(maxsize=None)
def reference(name):
    """(slots [nq][k] int32, dists [nq][k] f32) by the definition."""
    c = cases()[name]
    slots = np.full((c.nq, c.k), -1, dtype=np.int32)
    dists = np.full((c.nq, c.k), FLT_MAX, dtype=np.float32)
    for q in range(c.nq):
        r = c.row(q)
        key = (f2u(r).astype(np.uint64) << np.uint64(32)) | \
            np.arange(r.size, dtype=np.uint64)
        top = np.sort(key)[:c.k]
        idx = (top & np.uint64(0xFFFFFFFF)).astype(np.int64)
        slots[q, :idx.size] = idx
        dists[q, :idx.size] = r[idx]
    slots.setflags(write=False)
    dists.setflags(write=False)
    return slots, dists


def simulate(row: np.ndarray, k: int):
    """The filter's rule applied to one row: None when the row does not take
    the filter path, else (collected, falls_back)."""
    p = plan(row.size, k)
    if not p["filter"]:
        return None
    u = f2u(row)
    thr = np.sort(u[sample_positions(row.size, k)])[p["rank"] - 1]
    got = int((u <= thr).sum())
    return got, (got < k or got > p["capacity"])


@lru_cache(maxsize=None)
def expected_fallbacks(name) -> int:
    c = cases()[name]
    sims = [simulate(c.row(q), c.k) for q in range(c.nq)]
    return sum(1 for s in sims if s is not None and s[1])
