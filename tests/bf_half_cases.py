"""Case table of the f16 row store of the resident brute-force index
(BruteForceIndex(storage="f16"), moann_bf_new_typed in include/moann.h),
shared by tests/test_bf_half_ref.py (CPU) and tests/test_bf_half_gpu.py. It
extends tests/bf_cases.py, whose inputs, reference and bounds it reuses.

Exact cases. Integers in [-8, 8] are exact in binary16, their products are
exact, and every sum stays below 2^24, so the f64 reference of bf_cases, cast
to f32, is the expected bit pattern on an f16 store too, ties included: every
case of bc.EXACT is reused as it is. The new cases add the dims at which the
f16 kernel changes path: 8-half units (dim 7, 8), the second K=32 MFMA step
(33), the second and third 64-half slab (65, 129), a slab tail of one unit
(72), and long rows (127, 200). `quarter` has coordinates that are multiples
of 1/4 in [-2, 2] (products multiples of 1/16, still exact): a real f16
fraction, not only an integer, is converted and paired correctly. Four more
cases restate the corruption cases of bc.CORRUPTION_CASES at dim 65.

Float cases. Every case of bc.FLOAT, with the reference taken on the ROUNDED
inputs (X.astype(float16).astype(float32), the same for Q): an f16 index is
exact with respect to what it stores. The bounds are bc.dist_tol's on the
rounded arrays: f16 products are exact in f32, so the f16 MFMA's f32
accumulation is an f32 summation of exact terms in some order, which the
gamma(d) bounds cover."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

import bf_cases as bc
from bf_cases import (Case, KMAX, NEAR_TIE_CAP, TILE, dist_matrix, dist_tol,
                      filter_words, kernel_model, topk_of)

F32_MAX = bc.F32_MAX
_EDGE_BITS = (31, 32, 63, 64, 127, 128)

# ------------------------------ exact cases --------------------------------
NEW_EXACT = [
    Case("h_d7", 129, 129, 7, 10),                      # pads to one unit
    Case("h_d8", 129, 129, 8, 10),                      # one unit, no padding
    Case("h_d33_kmax", 300, 129, 33, KMAX, slice_rows=TILE),  # 2nd K=32 step
    Case("h_d65", 300, 129, 65, 10),                    # first unit of slab 2
    Case("h_d72_k1", 300, 257, 72, 1),                  # 8-half slab tail
    Case("h_d127_ip", 300, 129, 127, 10, metric="ip"),
    Case("h_d129_l2", 300, 129, 129, 10, metric="l2"),  # three slabs
    Case("h_d200_kmax", 300, 127, 200, KMAX, slice_rows=TILE),
    Case("h_d200_kbig", 300, 127, 200, KMAX + 1),       # gemm only
    Case("h_quarter", 300, 129, 72, 10, kind="quarter"),
]

# bc.CORRUPTION_CASES' four cases, restated at dim 65
CORRUPTION_CASES = {
    "le": Case("h_same300_d65", 300, 127, 65, 10, kind="same",
               slice_rows=TILE),
    "dist_only": Case("h_dup4_d65", 300, 129, 65, 10, kind="dup4",
                      slice_rows=TILE),
    "tail": Case("h_n129_d65", 129, 129, 65, 10, seed=1),
    "bitword": Case("h_flt_edges_d65", 300, 129, 65, KMAX, cleared=_EDGE_BITS,
                    kind="same"),
}

NEW = NEW_EXACT + list(CORRUPTION_CASES.values())
EXACT = bc.EXACT + NEW
FLOAT = bc.FLOAT
BY_NAME = {c.name: c for c in EXACT + FLOAT}
assert len(BY_NAME) == len(EXACT) + len(FLOAT)
_NEW_NAMES = {c.name for c in NEW}


@lru_cache(maxsize=None)
def inputs(name):
    """(X [n][dim] f32, Q [nq][dim] f32, ids [n] int64); bc.inputs for a case
    of bf_cases, bc.inputs' integer kinds and `quarter` for a new one."""
    if name not in _NEW_NAMES:
        return bc.inputs(name)
    c = BY_NAME[name]
    rng = np.random.Generator(np.random.PCG64(bc._seed("bfh", c.kind, c.n,
                                                       c.dim, c.seed)))
    if c.kind == "quarter":
        Q = rng.integers(-8, 9, (c.nq, c.dim)) / 4.0
        X = rng.integers(-8, 9, (c.n, c.dim)) / 4.0
    else:
        Q = rng.integers(-8, 9, (c.nq, c.dim))
        if c.kind == "same":
            X = np.repeat(rng.integers(-8, 9, (1, c.dim)), c.n, 0)
        elif c.kind == "dup4":
            base = rng.integers(-8, 9, (c.n // 4, c.dim))
            X = np.concatenate([base] * 4, 0)
        else:
            assert c.kind == "int", c.kind
            X = rng.integers(-8, 9, (c.n, c.dim))
    X, Q = X.astype(np.float32), Q.astype(np.float32)
    ids = np.arange(c.n, dtype=np.int64)
    for a in (X, Q, ids):
        a.setflags(write=False)
    return X, Q, ids


def to_half(a):
    """Round to binary16 (numpy: nearest even) and widen back, exactly."""
    return a.astype(np.float16).astype(np.float32)


@lru_cache(maxsize=None)
def stored(name):
    """(Xh, Qh, ids): what an f16 index stores and compares. Exact cases are
    unchanged by the rounding (test_bf_half_ref.py asserts it)."""
    X, Q, ids = inputs(name)
    Xh, Qh = to_half(X), to_half(Q)
    for a in (Xh, Qh):
        a.setflags(write=False)
    return Xh, Qh, ids


@lru_cache(maxsize=None)
def dist64(name):
    """[nq][n] f64 distances over the stored values; 'l2' is sqrt(l2sq)."""
    c = BY_NAME[name]
    Xh, Qh, _ = stored(name)
    if c.metric == "l2":
        D = np.sqrt(dist_matrix(Qh, Xh, "l2sq"))
    else:
        D = dist_matrix(Qh, Xh, c.metric)
    D.setflags(write=False)
    return D


@lru_cache(maxsize=None)
def tol(name):
    c = BY_NAME[name]
    Xh, Qh, _ = stored(name)
    t = dist_tol(Xh, Qh, c.metric)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def reference(name, k=None):
    """(ids, rows, f64 dists) [nq][k] by bc.topk_of over the stored values."""
    c = BY_NAME[name]
    return topk_of(dist64(name), bc.allowed_mask(c), stored(name)[2],
                   k or c.k)


def check_exact(name, ids, dists, ctx):
    """bc.check_exact's rule against `reference`: ids equal, l2sq / ip
    distances equal as f32 bit patterns, l2 within 1 ulp of the correctly
    rounded root."""
    c = BY_NAME[name]
    ref_ids, _, ref_d = reference(name)
    ref32 = ref_d.astype(np.float32)
    assert ids.shape == ref_ids.shape and dists.shape == ref_ids.shape, ctx
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


def near_tie_ranks(name):
    """bc.near_tie_ranks over the stored values: (count, ranks)."""
    c = BY_NAME[name]
    _, rows, d = reference(name, c.k + 1)
    t = tol(name)
    skip = bc.exact_queries(c)
    count = 0
    for q in range(c.nq):
        if q in skip:
            continue
        for r in range(c.k):
            if rows[q, r + 1] < 0:
                break
            pair = t[q, rows[q, r]] + t[q, rows[q, r + 1]]
            if d[q, r + 1] - d[q, r] <= pair:
                count += 1
    return count, (c.nq - len(skip)) * c.k


def check_float(name, ids, dists, ctx, ordered_ties=True):
    """bc.check_float's rules, over the stored values:

    - every distance is within dist_tol of the f64 distance of the row it is
      returned with;
    - no id repeats within a query, padding only where the reference pads;
    - an id differs from the reference's at a rank only in a near-tie: the
      f64 distances of the two rows differ by at most the sum of their
      dist_tol bounds;
    - differing ranks stay under NEAR_TIE_CAP of the case's ranks;
    - the exact queries (zero query under cosine) match exactly; with
      ordered_ties they return rows 0..k-1.

    Returns (differing ranks, ranks, worst error as a fraction of its
    bound)."""
    c = BY_NAME[name]
    all_ids = stored(name)[2]
    D, t = dist64(name), tol(name)
    ref_ids, ref_rows, _ = reference(name)
    assert ids.shape == ref_ids.shape and dists.shape == ref_ids.shape, ctx
    row_of = {int(v): i for i, v in enumerate(all_ids)}
    exact_q = bc.exact_queries(c)
    differing = 0
    worst = 0.0
    for q in range(c.nq):
        got = ids[q].tolist()
        real = [i for i in got if i >= 0]
        assert len(set(real)) == len(real), (ctx, "repeated id", q, got)
        assert [i >= 0 for i in got] == [i >= 0 for i in ref_ids[q].tolist()], \
            (ctx, "padding", q, got)
        if q in exact_q:
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
            worst = max(worst, err / t[q, row])
            assert err <= t[q, row], (ctx, "distance", q, r, i,
                                      float(dists[q, r]), D[q, row],
                                      t[q, row])
            if i != ref_ids[q, r]:
                differing += 1
                rr = ref_rows[q, r]
                gap = abs(D[q, row] - D[q, rr])
                assert gap <= t[q, row] + t[q, rr], (
                    ctx, "id beyond a near-tie", q, r, i, int(ref_ids[q, r]),
                    D[q, row], D[q, rr], t[q, row] + t[q, rr])
    ranks = (c.nq - len(exact_q)) * c.k
    print(f"{ctx}: {differing} of {ranks} ranks differ from the reference; "
          f"worst distance error {worst:.3f} of its bound")
    assert differing <= NEAR_TIE_CAP * ranks, (ctx, differing, ranks)
    return differing, ranks, worst
