"""The f16 row store of the resident brute-force index
(engine.BruteForceIndex(storage="f16"), moann_bf_new_typed / moann_bf_add_half
in include/moann.h) against the f64 reference of tests/bf_half_cases.py, in
both modes: the fused kernel on the f16 MFMA and the rank-GEMM + launch_topk
composition over a widened slice.

Exact cases (integer or quarter coordinates: exact in binary16, every f32
operation exact) must match the reference bit for bit, ties included. Float
cases are held to the format-derived bounds of bf_cases.dist_tol, taken on
the ROUNDED inputs: an f16 index is exact with respect to what it stores.
tests/test_bf_half_ref.py shows on the CPU that those cases have too few
near-ties for the excuse cap to hide a wrong result."""

import numpy as np
import pytest

import bf_cases as bc
import bf_half_cases as hc

pytestmark = pytest.mark.gpu


def _modes(c):
    """Modes that serve the case's k; `auto` where the planner chooses."""
    return (["fused", "gemm", "auto"] if c.k <= bc.KMAX else ["gemm", "auto"])


def _index(c, mode, storage="f16"):
    from matrixone_amd import engine
    X, _, ids = hc.inputs(c.name)
    ix = engine.BruteForceIndex(c.dim, metric=c.metric, storage=storage)
    ix.add(X, ids=ids if c.custom_ids else None)
    for row in c.deleted:
        ix.delete(int(ids[row]))
    ix.set_params(mode, c.slice_rows)
    return ix


def _search(c, mode):
    ix = _index(c, mode)
    try:
        assert ix.storage == "f16"
        assert len(ix) == c.n  # deleted rows still count
        words = bc.filter_words(c) if c.filtered else None
        return ix.search(hc.inputs(c.name)[1], c.k, row_bitset=words)
    finally:
        ix.close()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name,mode", [(c.name, m) for c in hc.EXACT
                                       for m in _modes(c)])
def test_exact_case(name, mode):
    c = hc.BY_NAME[name]
    ids, dists = _search(c, mode)
    hc.check_exact(name, ids, dists, f"f16/{name}/{mode}")


@pytest.mark.parametrize("name,mode", [(c.name, m) for c in hc.FLOAT
                                       for m in _modes(c)[:2]])
def test_float_case(name, mode):
    c = hc.BY_NAME[name]
    ids, dists = _search(c, mode)
    # the gemm mode selects per distance tile with launch_topk, which keeps
    # row order among bit-equal distances up to 1024 candidates
    hc.check_float(name, ids, dists, f"f16/{name}/{mode}",
                   ordered_ties=mode == "fused" or c.n <= 1024)


def test_everything_excluded_is_all_padding():
    for mode in ("fused", "gemm"):
        ids, dists = _search(hc.BY_NAME["flt_all"], mode)
        assert (ids == -1).all() and (dists == bc.F32_MAX).all(), mode


# ------------------------- narrowing: nearest even -------------------------

def _rounding_rows():
    """300 x 40 Gaussian rows at five scales, from the binary16 subnormal
    range to just under its largest finite value, with halfway values
    planted: the two roundings must agree on every one of them."""
    rng = np.random.default_rng(16)
    scale = np.array([3e-7, 4e-5, 1.0, 100.0, 21000.0])[np.arange(300) % 5]
    X = (rng.standard_normal((300, 40)) * scale[:, None]).astype(np.float32)
    X = np.clip(X, -65519.0, 65519.0)
    ties = np.array([
        1 + 2.0 ** -11,        # halfway, down to the even 1
        1 + 3 * 2.0 ** -11,    # halfway, up to the even 1 + 2^-9
        -(1 + 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0,
        2.0 ** -25,            # halfway between 0 and the least subnormal
        3 * 2.0 ** -25,        # halfway between two subnormals
        2.0 ** -14 - 2.0 ** -25,  # rounds up to the least normal
        65519.0, -65519.0,     # the largest values that stay finite: 65504
        65504.0 - 16.0 + 1e-3, 65488.0,  # just past / on a halfway point
    ], dtype=np.float32)
    X[2, :ties.size] = ties
    X[7, 40 - ties.size:] = -ties
    assert np.isfinite(X.astype(np.float16)).all()
    h = X.astype(np.float16)
    assert (h.astype(np.float32) != X).mean() > 0.9  # rounding does happen
    assert (h[::5] != 0).any() and (np.abs(h[::5]) < 2.0 ** -14).all()
    assert np.abs(h).max() == 65504.0
    return X


@pytest.mark.parametrize("metric", ["l2sq", "ip", "cos"])
def test_narrowing_is_round_to_nearest_even(metric):
    """Index A narrows f32 rows on the device, index B is given numpy's
    float16 cast (nearest even) through moann_bf_add_half: byte-identical
    results in both modes. The unit-vector queries return -x_j under ip, so a
    single coordinate rounded the other way shows."""
    from matrixone_amd import engine
    X = _rounding_rows()
    Q = np.concatenate([np.eye(40, dtype=np.float32),
                        X[3:20] * np.float32(0.001)])
    sub = np.zeros(10, dtype=np.uint32)  # bits of rows 0, 5, 10, ...
    for r in range(0, 300, 5):
        sub[r >> 5] |= np.uint32(1 << (r & 31))
    res = {}
    for tag, rows in (("f32", X), ("f16", X.astype(np.float16))):
        ix = engine.BruteForceIndex(40, metric=metric, storage="f16")
        try:
            ix.add(rows)
            for mode in ("fused", "gemm"):
                ix.set_params(mode, 0)
                res[tag, mode] = ix.search(Q, bc.KMAX)
            if metric == "ip":  # every row of every coordinate: k = n
                ix.set_params("gemm", 0)
                res[tag, "all"] = ix.search(Q[:40], 300)
                # and the 60 rows of the subnormal range through the fused
                # kernel: the f16 MFMA must take subnormal operands as they are
                ix.set_params("fused", 0)
                res[tag, "sub"] = ix.search(Q[:40], 60, row_bitset=sub)
        finally:
            ix.close()
    for mode in ("fused", "gemm"):
        assert _same(res["f32", mode], res["f16", mode]), mode
    if metric == "ip":
        assert _same(res["f32", "all"], res["f16", "all"])
        want = np.sort(-X.astype(np.float16).astype(np.float32).T, axis=1)
        np.testing.assert_array_equal(res["f32", "all"][1], want)
        assert _same(res["f32", "sub"], res["f16", "sub"])
        want = np.sort(-X[::5].astype(np.float16).astype(np.float32).T, axis=1)
        assert (want != 0).mean() > 0.9
        np.testing.assert_array_equal(res["f32", "sub"][1], want)


# ------------------------------ refusals -----------------------------------

def test_out_of_range_is_refused_and_stores_nothing():
    from matrixone_amd import engine
    X, Q, _ = hc.inputs("n300")
    ix = engine.BruteForceIndex(64, storage="f16")
    try:
        ix.add(X[:100])
        before = ix.search(Q, 10)
        for bad, dtype in ((70000.0, np.float32), (np.inf, np.float32),
                           (65520.0, np.float32), (np.nan, np.float32),
                           (np.inf, np.float16), (np.nan, np.float16)):
            rows = X[100:110].astype(dtype)
            rows[6, 63] = bad
            with pytest.raises(engine.MoannError, match="row 6 .*f16"):
                ix.add(rows)
            assert len(ix) == 100, (bad, dtype)
        edge = X[100:101].copy()
        edge[0, 0] = np.float32(65519.996)  # the largest f32 below 65520
        assert np.isfinite(edge.astype(np.float16)).all()
        probe = engine.BruteForceIndex(64, storage="f16")
        probe.add(edge)
        assert len(probe) == 1
        probe.close()
        for mode in ("fused", "gemm"):
            ix.set_params(mode, 0)
            bad_q = np.array(Q[:5])
            bad_q[3, 0] = 1e6
            with pytest.raises(engine.MoannError, match="query 3 .*f16"):
                ix.search(bad_q, 10)
            with pytest.raises(engine.MoannError, match="query 3 .*f16"):
                ix.search(bad_q, 10, row_bitset=np.full(4, 0xFFFFFFFF,
                                                        dtype=np.uint32))
        ix.set_params("auto", 0)
        assert _same(ix.search(Q, 10), before)  # nothing was stored
    finally:
        ix.close()


def test_storage_types():
    from matrixone_amd import engine
    X, _, _ = hc.inputs("n300")
    with pytest.raises(engine.MoannError, match="Quantization_F32 or "
                                                "Quantization_F16"):
        engine.BruteForceIndex(64, storage="int8")
    with pytest.raises(engine.MoannError, match="Quantization_F32 or "
                                                "Quantization_F16"):
        engine.BruteForceIndex(64, storage="bf16")
    with pytest.raises(engine.MoannError):
        engine.BruteForceIndex(64, storage="f64")
    ix = engine.BruteForceIndex(64)
    try:
        assert ix.storage == "f32"
        with pytest.raises(engine.MoannError, match="stores f32"):
            ix.add_half(X[:10].astype(np.float16))
        assert len(ix) == 0
        ix.add(X[:10].astype(np.float16))  # an f32 index widens any dtype
        assert len(ix) == 10
    finally:
        ix.close()


def test_f32_storage_is_the_old_path():
    """BruteForceIndex(storage="f32") returns byte for byte what
    BruteForceIndex() returns."""
    from matrixone_amd import engine
    X, Q, _ = hc.inputs("n300")
    got = {}
    for tag, kw in (("default", {}), ("f32", {"storage": "f32"})):
        ix = engine.BruteForceIndex(64, **kw)
        try:
            assert ix.storage == "f32"
            ix.add(X)
            for mode in ("fused", "gemm"):
                ix.set_params(mode, 0)
                got[tag, mode] = ix.search(Q, 10)
        finally:
            ix.close()
    for mode in ("fused", "gemm"):
        assert _same(got["default", mode], got["f32", mode])
        bc.check_exact("n300", *got["f32", mode], f"f32/{mode}")


# ------------------- append, device queries, perf, tail --------------------

@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("mode", ["fused", "gemm"])
def test_append_equals_a_fresh_index(mode, custom):
    """100 rows, a search, 200 more (the capacity of 128 grows to 512 on the
    way, a device-to-device copy of 2-byte elements), a search: byte for byte
    what a fresh index over the 300 returns."""
    from matrixone_amd import engine
    X, Q, _ = hc.inputs("n300")
    ids = (5000 - 3 * np.arange(300, dtype=np.int64)) if custom else None
    cut = lambda a, lo, hi: None if a is None else a[lo:hi]

    def fresh(nrows):
        ix = engine.BruteForceIndex(64, capacity=nrows, storage="f16")
        ix.set_params(mode, 0)
        ix.add(X[:nrows], ids=cut(ids, 0, nrows))
        try:
            return ix.search(Q, 10)
        finally:
            ix.close()

    ix = engine.BruteForceIndex(64, storage="f16")
    try:
        ix.set_params(mode, 0)
        ix.add(X[:100], ids=cut(ids, 0, 100))
        first = ix.search(Q, 10)
        ix.add(X[100:].astype(np.float16), ids=cut(ids, 100, 300))
        assert len(ix) == 300
        second = ix.search(Q, 10)
    finally:
        ix.close()
    for got, want in ((first, fresh(100)), (second, fresh(300))):
        assert _same(got, want)
    ref = hc.reference("n300")[1]
    assert (second[0] == (ref if ids is None else ids[ref])).all()


@pytest.mark.parametrize("mode", ["fused", "gemm"])
def test_device_queries_and_perf(mode):
    import torch
    c = hc.BY_NAME["h_d65"]
    ix = _index(c, mode)
    try:
        Q = hc.inputs(c.name)[1]
        p0 = ix.perf()
        host = ix.search(Q, c.k)
        p1 = ix.perf()
        qd = torch.from_numpy(np.array(Q)).cuda()
        torch.cuda.synchronize()
        dev = ix.search_device(qd, c.k)
        assert _same(host, dev)
        hc.check_exact(c.name, *dev, f"device/{mode}")
        assert p1["scan_bytes"] - p0["scan_bytes"] == c.n * c.dim * 2
        assert p1["scan_rows"] - p0["scan_rows"] == c.n * c.nq
        assert p1["scan_ms"] > p0["scan_ms"]
        assert set(p1) == set(_index_perf_fields())
        empty = ix.search(Q[:0], c.k)  # nq = 0 returns at once
        assert empty[0].shape == (0, c.k)
    finally:
        ix.close()


def _index_perf_fields():
    from matrixone_amd import engine
    ix = engine.BruteForceIndex(4)
    try:
        return list(ix.perf())
    finally:
        ix.close()


def test_search_with_tail_takes_an_f16_tail():
    """search_with_tail(tail_index=<f16 index>) equals the tail_vecs form, on
    the integer inputs of tests/test_bf_gpu.py's tail test."""
    from matrixone_amd import engine
    rng = np.random.default_rng(12)
    X = rng.integers(-8, 9, (400, 16)).astype(np.float32)
    Q = rng.integers(-8, 9, (37, 16)).astype(np.float32)
    T = rng.integers(-8, 9, (50, 16)).astype(np.float32)
    t_ids = 10000 + np.arange(50, dtype=np.int64)
    C = X[:4].copy()
    assign = bc.dist_matrix(X, C, "l2sq").argmin(1).astype(np.int32)
    main = engine.IvfFlatIndex(16, 4, metric="l2sq", capacity=400)
    tail = engine.BruteForceIndex(16, storage="f16")
    try:
        main.add(X, ids=np.arange(400, dtype=np.int64))
        main.set_centroids(C)
        main.set_assignments(assign)
        main.build()
        tail.add(T[:20], ids=t_ids[:20])
        tail.add(T[20:].astype(np.float16), ids=t_ids[20:])
        want = engine.search_with_tail(main, Q, 10, 4, T, t_ids)
        got = engine.search_with_tail(main, Q, 10, 4, None, None,
                                      tail_index=tail)
        assert (want[0] >= 10000).any()  # the tail does reach the results
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    finally:
        main.close()
        tail.close()
