"""Case table shared by tests/test_bf_cases_ref.py (CPU self-test of the
reference and of the checks) and tests/test_bf_gpu.py (the resident
brute-force index, include/moann.h "resident brute force", against that
reference). Inputs are seeded and small; every reference is computed once
per process and shared.

Reference: `dist_matrix` of tests/test_kmeans_gpu.py in f64, then a lexsort
by (distance, row) over the rows that are neither deleted nor filtered, ids
mapped, (-1, f32 max) padding.

Exact cases have integer coordinates in [-8, 8] and dim <= 64: every product,
sum and norm is an integer below 2^24, so each f32 operation of the kernels
is exact and the f64 reference, cast to f32, is the expected bit pattern.
Float cases are checked with bounds derived from the number formats
(`dist_tol`), never from what the GPU returns."""

from __future__ import annotations

import bisect
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from test_kmeans_gpu import dist_matrix, gamma

F32_MAX = np.finfo(np.float32).max
TILE = 128   # rows per tile and slice granule (moann_bf_plan.h BF_TILE)
KMAX = 64    # moann_bf_fused_kmax(); test_bf_gpu.py asserts the library agrees
U = 2.0 ** -24
NEAR_TIE_CAP = 0.01  # of the ranks of a float case


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    nq: int
    dim: int
    k: int
    metric: str = "l2sq"
    kind: str = "int"        # int | dup4 | same | mix
    slice_rows: int = 0      # 0 = planner
    cleared: tuple = ()      # rows whose filter bit is cleared; () = no filter
    deleted: tuple = ()      # ROWS deleted (by their id) before the search
    custom_ids: bool = False
    seed: int = 0

    @property
    def exact(self):
        return self.kind != "mix"

    @property
    def filtered(self):
        return bool(self.cleared)


ALL = "all"  # `cleared` value: every bit cleared

# ------------------------------ exact cases --------------------------------
# n in {1, 127, 128, 129, 300}, nq in {1, 127, 129, 257}, dim in
# {1, 3, 4, 33, 36, 64}, k in {1, 10, KMAX, KMAX+1}; with n <= 300 and
# k <= KMAX+1 every selection sees at most 3 * 65 candidates, inside
# launch_topk's position-ordered range.
EXACT = [
    Case("n1", 1, 1, 1, 1),
    Case("n1_k10", 1, 127, 3, 10),                       # k > n: padding
    Case("n127", 127, 129, 4, 10),
    Case("n128", 128, 127, 33, KMAX),
    Case("n129", 129, 129, 36, 10, seed=1),              # 1-row second tile
    Case("n129_kbig", 129, 1, 64, KMAX + 1),             # gemm only
    Case("n300", 300, 257, 64, 10),
    Case("n300_k1", 300, 257, 33, 1),
    Case("n300_kmax", 300, 129, 36, KMAX),
    Case("n300_kbig", 300, 127, 3, KMAX + 1),
    Case("n300_ip", 300, 129, 33, 10, metric="ip"),
    Case("n300_l2", 300, 129, 36, 10, metric="l2"),
    Case("n127_ip_kmax", 127, 257, 4, KMAX, metric="ip"),
    Case("n40_k64", 40, 129, 4, KMAX),                   # k > n, fused lists
    Case("slices3", 300, 129, 64, 10, slice_rows=TILE),  # 128 + 128 + 44
    Case("slices3_kmax", 300, 127, 1, KMAX, slice_rows=TILE),
    Case("slices3_kbig", 300, 127, 3, KMAX + 1, slice_rows=TILE),
    Case("dup4", 300, 129, 33, 10, kind="dup4", slice_rows=TILE),
    Case("dup4_auto", 300, 257, 4, KMAX, kind="dup4"),
    Case("same300", 300, 127, 36, 10, kind="same", slice_rows=TILE),
    Case("ids", 300, 129, 33, 10, custom_ids=True),
    # filter and delete
    # identical rows: the result is the first k surviving rows, so a cleared
    # bit that is ignored, or read from the wrong word, shows at once
    Case("flt_edges", 300, 129, 33, KMAX, cleared=(31, 32, 63, 64, 127, 128),
         kind="same"),
    Case("flt_edges_kbig", 300, 127, 33, 140,
         cleared=(31, 32, 63, 64, 127, 128), kind="same"),   # gemm only
    Case("flt_edges_int", 300, 129, 3, KMAX,
         cleared=(31, 32, 63, 64, 127, 128), slice_rows=TILE),
    Case("flt_all", 300, 129, 4, 10, cleared=ALL),
    Case("flt_few", 300, 129, 4, 10,
         cleared=tuple(r for r in range(300) if r not in (5, 130, 131, 257, 299))),
    Case("del", 300, 129, 33, 10, deleted=(0, 127, 128, 299), custom_ids=True),
    Case("del_and_flt", 300, 129, 33, KMAX, deleted=(0, 64, 128),
         cleared=(1, 64, 129, 256), kind="same"),
    Case("del_and_flt_int", 300, 129, 3, KMAX, deleted=(0, 64, 128),
         cleared=(1, 64, 129, 256), slice_rows=TILE),
]

# ------------------------------ float cases --------------------------------
# Gaussian mixtures, nq = 64, all four metrics. Under cosine row 7 is a zero
# row and query 3 a zero query (distance exactly 1 to everything).
FLOAT = [
    Case(f"mix{n}x{d}_{m}", n, 64, d, k, metric=m, kind="mix", seed=s)
    for (n, d, k, s) in ((1000, 100, 10, 0), (500, 33, 10, 0),
                         (2000, 768, 10, 0))
    for m in ("l2sq", "l2", "ip", "cos")
] + [
    Case("mix500x33_kmax", 500, 64, 33, KMAX, kind="mix"),
    Case("mix500x33_kbig", 500, 64, 33, KMAX + 1, kind="mix"),
    Case("mix500x33_slices", 500, 64, 33, 10, kind="mix", slice_rows=TILE),
]

CASES = EXACT + FLOAT
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

ZERO_ROW, ZERO_QUERY = 7, 3


def scale_mixture(n, dim, ncomp, seed, k):
    """A Gaussian scale mixture: row i is drawn around centre i % ncomp
    (uniform in [-1, 1]^dim) with variance 0.01 * g^l, l = i // ncomp its
    level and g = 30^(1/(k+2)). A query that is a near copy of a level-0 row
    finds the rows of its own component at squared distances of about
    dim * (0.01 + 0.01 g^l), a factor g apart, and levels 0..k+1 all lie
    below the rows of the other components (from dim * 2/3 on), which crowd
    together. With equal variances the top ranks are a sqrt(8/dim) apart at
    best, and the worst-case f32 bounds at dim 768 turn several percent of
    them into near-ties: the excuse cap of the GPU test (NEAR_TIE_CAP) would
    mean nothing."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-1.0, 1.0, (ncomp, dim))
    g = 30.0 ** (1.0 / (k + 2))
    sig = np.sqrt(0.01 * g ** (np.arange(n) // ncomp))
    X = centers[np.arange(n) % ncomp] + \
        sig[:, None] * rng.standard_normal((n, dim))
    return X.astype(np.float32)


@lru_cache(maxsize=None)
def inputs(name):
    """(X [n][dim] f32, Q [nq][dim] f32, ids [n] int64)."""
    c = BY_NAME[name]
    rng = np.random.Generator(np.random.PCG64(_seed("bf", c.kind, c.n, c.dim,
                                                    c.seed)))
    if c.kind == "mix":
        # 20 levels per component, 100 where k is large; query i is a near
        # copy of row i, which is of level 0 (ncomp >= nq) or 1
        ncomp = c.n // (100 if c.k > 10 else 20)
        X = scale_mixture(c.n, c.dim, ncomp, 40 + c.seed + c.dim, c.k)
        if c.metric == "ip":
            # inner products do not order by the noise level: the rows of
            # level l are scaled by 1 + 0.1 * (L-1-l), so that a query's
            # products with its own component, about |centre|^2 times that
            # factor, descend level by level
            level = np.arange(c.n) // ncomp
            X = X * (1.0 + 0.1 * (level.max() - level))[:, None].astype(
                np.float32)
        Q = X[:c.nq] + np.float32(0.01)
        if c.metric == "cos":
            X = X.copy()
            Q = Q.copy()
            X[ZERO_ROW] = 0
            Q[ZERO_QUERY] = 0
    else:
        Q = rng.integers(-8, 9, (c.nq, c.dim)).astype(np.float32)
        if c.kind == "same":
            X = np.repeat(rng.integers(-8, 9, (1, c.dim)), c.n, 0)
        elif c.kind == "dup4":
            # every vector 4 times, the copies n/4 rows apart: they straddle
            # the tile and slice boundaries at 128 and 256
            base = rng.integers(-8, 9, (c.n // 4, c.dim))
            X = np.concatenate([base] * 4, 0)
        else:
            X = rng.integers(-8, 9, (c.n, c.dim))
        X = X.astype(np.float32)
    if c.custom_ids:
        ids = 1000 + 7 * rng.permutation(c.n).astype(np.int64)
    else:
        ids = np.arange(c.n, dtype=np.int64)
    for a in (X, Q, ids):
        a.setflags(write=False)
    return X, Q, ids


def cleared_rows(c):
    return tuple(range(c.n)) if c.cleared == ALL else c.cleared


def filter_words(c):
    """The row_bitset a filtered case passes: all bits set but the cleared."""
    w = np.full((c.n + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)
    for r in cleared_rows(c):
        w[r >> 5] &= np.uint32(~(1 << (r & 31)) & 0xFFFFFFFF)
    return w


def allowed_mask(c):
    m = np.ones(c.n, dtype=bool)
    m[np.array(cleared_rows(c), dtype=np.int64)] = False
    m[np.array(c.deleted, dtype=np.int64)] = False
    return m


@lru_cache(maxsize=None)
def dist64(name):
    """[nq][n] f64 distances of the case's metric; 'l2' is sqrt(l2sq)."""
    c = BY_NAME[name]
    X, Q, _ = inputs(name)
    if c.metric == "l2":
        D = np.sqrt(dist_matrix(Q, X, "l2sq"))
    else:
        D = dist_matrix(Q, X, c.metric)
    D.setflags(write=False)
    return D


def topk_of(D, allowed, ids, k):
    """lexsort by (distance, row) over the allowed rows -> ids [nq][k] int64,
    rows [nq][k], dists [nq][k] f64, (-1, -1, f32 max) padding."""
    nq = D.shape[0]
    rows = np.nonzero(allowed)[0]
    out_r = np.full((nq, k), -1, dtype=np.int64)
    out_d = np.full((nq, k), float(F32_MAX), dtype=np.float64)
    m = min(k, rows.size)
    for q in range(nq):
        order = rows[np.lexsort((rows, D[q, rows]))][:m]
        out_r[q, :m] = order
        out_d[q, :m] = D[q, order]
    out_i = np.where(out_r >= 0, ids[np.maximum(out_r, 0)], -1)
    return out_i, out_r, out_d


@lru_cache(maxsize=None)
def reference(name, k=None):
    c = BY_NAME[name]
    _, _, ids = inputs(name)
    return topk_of(dist64(name), allowed_mask(c), ids, k or c.k)


# ---------------- the kernel, restated with python lists -------------------

def kernel_model(D, words, k, slice_rows, corrupt=None):
    """Per-slice partial top-k with strict-< insertion in ascending row
    order, then a merge of the position-ordered candidates: what
    bf_fused_topk_kernel + launch_topk + the gather compute, on a given
    [nq][n] distance matrix and bitset words (alive AND filter). Returns rows
    [nq][k] (-1 padding) and distances (f32 max padding).

    corrupt: None, or one seeded defect —
      "le"        <= instead of < (an equal later row displaces an earlier)
      "dist_only" merge by distance only (position order among equals lost)
      "tail"      the rows of a slice's last, partial tile are dropped
      "bitword"   the bit is read from the next bitset word"""
    nq, n = D.shape
    out_r = np.full((nq, k), -1, dtype=np.int64)
    out_d = np.full((nq, k), float(F32_MAX), dtype=np.float64)
    bounds = list(range(0, n, slice_rows)) + [n]

    def passes(row):
        w = row >> 5
        if corrupt == "bitword":
            w = min(w + 1, len(words) - 1)
        return (int(words[w]) >> (row & 31)) & 1

    for q in range(nq):
        cand = []  # position-ordered (dist, row), each slice padded to k
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if corrupt == "tail":
                hi = lo + (hi - lo) // TILE * TILE
            ds, rs = [], []
            for row in range(lo, hi):
                if not passes(row):
                    continue
                d = D[q, row]
                if not d < F32_MAX:
                    continue
                if len(ds) == k:
                    if not (d <= ds[-1] if corrupt == "le" else d < ds[-1]):
                        continue
                # behind its equals: the new row is larger than every listed
                pos = (bisect.bisect_left if corrupt == "le"
                       else bisect.bisect_right)(ds, d)
                ds.insert(pos, d)
                rs.insert(pos, row)
                del ds[k:], rs[k:]
            cand += list(zip(ds, rs)) + [(float(F32_MAX), -1)] * (k - len(ds))
        if corrupt == "dist_only":
            order = sorted(range(len(cand)), key=lambda i: (cand[i][0], -i))
        else:
            order = sorted(range(len(cand)), key=lambda i: (cand[i][0], i))
        for e, i in enumerate(order[:k]):
            if cand[i][1] >= 0:
                out_r[q, e], out_d[q, e] = cand[i][1], cand[i][0]
    return out_r, out_d


def alive_and_filter_words(c):
    w = filter_words(c) if c.filtered else np.full((c.n + 31) // 32,
                                                   0xFFFFFFFF, np.uint32)
    w = w.copy()
    for r in c.deleted:
        w[r >> 5] &= np.uint32(~(1 << (r & 31)) & 0xFFFFFFFF)
    return w


def model_slice_rows(c):
    """Slice length the model walks: the override, or one slice per tile (any
    whole-tile slicing must give the same result; one tile is the finest)."""
    return c.slice_rows or TILE


# corruption -> the exact case that must catch it
CORRUPTION_CASES = {
    "le": "same300",
    "dist_only": "dup4",
    "tail": "n129",
    "bitword": "flt_edges",
}

# ------------------------------ float checks -------------------------------

def dist_tol(X, Q, metric):
    """[nq][n] bound on |f32 distance - f64 distance| of one (query, row)
    pair: half of test_kmeans_gpu.assign_tol's two-distance figures.

    l2sq  2*gamma(d+2)*(|x|+|q|)^2: the dot product's gamma(d)*|x||q| doubled,
          plus the two norms and the final adds; it bounds the expanded and
          the difference form alike.
    ip    gamma(d)*|x||q|, one f32 fmaf chain.
    cos   2*gamma(d+2): gamma(d) from the dot, gamma(d)/2 from each norm's
          square root, 2u from the final rounding of 1 - sim.
    l2    the root of an l2sq value a within t of the true b:
          |sqrt(a)-sqrt(b)| = |a-b|/(sqrt(a)+sqrt(b)) <= min(sqrt(t),
          t/sqrt(b)), plus 2u*sqrt(b) for the f64 root rounded to f32."""
    d = X.shape[1]
    xn = np.sqrt((X.astype(np.float64) ** 2).sum(1))[None, :]
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(1))[:, None]
    if metric in ("l2sq", "l2"):
        t = 2.0 * gamma(d + 2) * (xn + qn) ** 2
        if metric == "l2sq":
            return t
        b = np.sqrt(dist_matrix(Q, X, "l2sq"))
        with np.errstate(divide="ignore"):
            return np.minimum(np.sqrt(t), t / b) + 2.0 * U * b
    if metric == "ip":
        return gamma(d) * xn * qn
    if metric == "cos":
        return np.full((Q.shape[0], X.shape[0]), 2.0 * gamma(d + 2))
    raise ValueError(metric)


def exact_queries(c):
    """Queries of a float case whose result is nevertheless exact: the zero
    query under cosine is at distance exactly 1.0f from every row in any
    arithmetic (mo_cos_distance returns 1 for a zero denominator), so its
    result is rows 0..k-1 at 1.0 and it takes no part in the near-tie
    excuse."""
    return (ZERO_QUERY,) if c.metric == "cos" and c.kind == "mix" else ()


def near_tie_ranks(name):
    """Ranks r < k of the reference top-(k+1) whose successor lies within
    what two f32 distances can differ by: the ranks at which a correct f32
    result may differ from the reference. Returns (count, ranks)."""
    c = BY_NAME[name]
    X, Q, _ = inputs(name)
    _, rows, d = reference(name, c.k + 1)
    tol = dist_tol(X, Q, c.metric)
    count = 0
    skip = exact_queries(c)
    for q in range(c.nq):
        if q in skip:
            continue
        for r in range(c.k):
            if rows[q, r + 1] < 0:
                break
            pair = tol[q, rows[q, r]] + tol[q, rows[q, r + 1]]
            if d[q, r + 1] - d[q, r] <= pair:
                count += 1
    return count, (c.nq - len(skip)) * c.k


def check_float(name, ids, dists, ctx, ordered_ties=True):
    """A float case's result against the reference. ordered_ties: the result
    comes from a path that resolves bit-equal distances to the lowest row
    (the fused kernel always; launch_topk while it selects among at most
    1024 candidates), so the exact queries must return rows
    0..k-1; otherwise any k distinct rows at distance exactly 1 will do.

    - every distance is within dist_tol of the f64 distance of the row it is
      returned with;
    - no id repeats within a query, padding only where the reference pads;
    - an id differs from the reference's at a rank only in a near-tie: the
      f64 distances of the two rows differ by at most the sum of their
      dist_tol bounds;
    - differing ranks stay under NEAR_TIE_CAP of the case's ranks;
    - the exact queries (zero query under cosine) match exactly."""
    c = BY_NAME[name]
    X, Q, all_ids = inputs(name)
    D = dist64(name)
    tol = dist_tol(X, Q, c.metric)
    ref_ids, ref_rows, ref_d = reference(name)
    assert ids.shape == ref_ids.shape and dists.shape == ref_ids.shape, ctx
    row_of = {int(v): i for i, v in enumerate(all_ids)}
    differing = 0
    worst = 0.0
    for q in range(c.nq):
        got = ids[q].tolist()
        real = [i for i in got if i >= 0]
        assert len(set(real)) == len(real), (ctx, "repeated id", q, got)
        assert [i >= 0 for i in got] == [i >= 0 for i in ref_ids[q].tolist()], \
            (ctx, "padding", q, got)
        if q in exact_queries(c):
            if ordered_ties:
                assert got == ref_ids[q].tolist(), (ctx, "zero query ids", q,
                                                    got)
            assert all(i in row_of for i in got), (ctx, "zero query ids", q)
            assert (dists[q] == np.float32(1.0)).all(), (ctx, q, dists[q])
            continue
        for r, i in enumerate(got):
            if i < 0:
                assert dists[q, r] == F32_MAX, (ctx, "padding distance", q, r)
                continue
            row = row_of[i]
            err = abs(float(dists[q, r]) - D[q, row])
            worst = max(worst, err / tol[q, row])
            assert err <= tol[q, row], (ctx, "distance", q, r, i,
                                        float(dists[q, r]), D[q, row],
                                        tol[q, row])
            if i != ref_ids[q, r]:
                differing += 1
                rr = ref_rows[q, r]
                gap = abs(D[q, row] - D[q, rr])
                assert gap <= tol[q, row] + tol[q, rr], (
                    ctx, "id beyond a near-tie", q, r, i, int(ref_ids[q, r]),
                    D[q, row], D[q, rr], tol[q, row] + tol[q, rr])
    ranks = (c.nq - len(exact_queries(c))) * c.k
    print(f"{ctx}: {differing} of {ranks} ranks differ from the reference; "
          f"worst distance error {worst:.3f} of its bound")
    assert differing <= NEAR_TIE_CAP * ranks, (ctx, differing, ranks)


def check_exact(name, ids, dists, ctx):
    """An exact case's result: ids equal, l2sq / ip distances equal as f32
    values, l2 within 1 ulp of the correctly rounded root."""
    c = BY_NAME[name]
    ref_ids, _, ref_d = reference(name)
    ref32 = ref_d.astype(np.float32)
    bad = np.argwhere(ids != ref_ids)
    assert bad.size == 0, (ctx, "ids", bad[:5].tolist(),
                           ids[tuple(bad[0])], ref_ids[tuple(bad[0])],
                           ids[bad[0][0]].tolist(),
                           ref_ids[bad[0][0]].tolist())
    if c.metric == "l2":
        real = ref_ids >= 0
        assert (np.abs(dists[real].astype(np.float64) -
                       ref32[real].astype(np.float64))
                <= np.spacing(ref32[real]).astype(np.float64)).all(), ctx
        assert (dists[~real] == F32_MAX).all(), ctx
    else:
        bad = np.argwhere(dists != ref32)
        assert bad.size == 0, (ctx, "distances", bad[:5].tolist(),
                               dists[tuple(bad[0])], ref32[tuple(bad[0])])
