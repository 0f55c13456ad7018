"""The resident brute-force index (engine.BruteForceIndex, moann_bf_* in
include/moann.h) against the f64 reference of tests/bf_cases.py, in both of
its modes: the fused MFMA distance + top-k kernel and the rank-GEMM +
launch_topk composition.

Exact cases (integer coordinates, every f32 operation exact) must match the
reference bit for bit, ties included: equal distances resolve to the row
added first. Float cases are held to bounds derived from the number formats
(bf_cases.dist_tol); tests/test_bf_cases_ref.py shows on the CPU that those
cases have too few near-ties for the excuse cap to hide a wrong result."""

import numpy as np
import pytest

import bf_cases as bc

pytestmark = pytest.mark.gpu


def _modes(c):
    """Modes that serve the case's k; `auto` where the planner chooses."""
    return (["fused", "gemm", "auto"] if c.k <= bc.KMAX else ["gemm", "auto"])


def _index(c, mode):
    from matrixone_amd import engine
    X, _, ids = bc.inputs(c.name)
    ix = engine.BruteForceIndex(c.dim, metric=c.metric)
    ix.add(X, ids=ids if c.custom_ids else None)
    for row in c.deleted:
        ix.delete(int(ids[row]))
    ix.set_params(mode, c.slice_rows)
    return ix


def _search(c, mode):
    ix = _index(c, mode)
    try:
        assert len(ix) == c.n  # deleted rows still count
        words = bc.filter_words(c) if c.filtered else None
        return ix.search(bc.inputs(c.name)[1], c.k, row_bitset=words)
    finally:
        ix.close()


def test_fused_kmax_is_the_tables():
    from matrixone_amd import engine
    assert engine.bf_fused_kmax() == bc.KMAX
    assert bc.KMAX >= 32


@pytest.mark.parametrize("name,mode", [(c.name, m) for c in bc.EXACT
                                       for m in _modes(c)])
def test_exact_case(name, mode):
    c = bc.BY_NAME[name]
    ids, dists = _search(c, mode)
    bc.check_exact(name, ids, dists, f"{name}/{mode}")


@pytest.mark.parametrize("name,mode", [(c.name, m) for c in bc.FLOAT
                                       for m in _modes(c)[:2]])
def test_float_case(name, mode):
    c = bc.BY_NAME[name]
    ids, dists = _search(c, mode)
    # the gemm mode selects per distance tile with launch_topk, which keeps
    # row order among bit-equal distances up to 1024 candidates
    bc.check_float(name, ids, dists, f"{name}/{mode}",
                   ordered_ties=mode == "fused" or c.n <= 1024)


@pytest.mark.parametrize("name", [c.name for c in bc.FLOAT])
def test_one_shot_entry_meets_the_same_reference(name):
    """engine.brute_force_search, the yardstick the resident index replaces
    for repeated searches, by the same rule."""
    from matrixone_amd import engine
    c = bc.BY_NAME[name]
    X, Q, _ = bc.inputs(name)
    ids, dists = engine.brute_force_search(X, Q, c.k, metric=c.metric)
    bc.check_float(name, ids, dists, f"{name}/one-shot",
                   ordered_ties=c.n <= 1024)


def test_everything_excluded_is_all_padding():
    for mode in ("fused", "gemm"):
        ids, dists = _search(bc.BY_NAME["flt_all"], mode)
        assert (ids == -1).all() and (dists == bc.F32_MAX).all(), mode


def test_filter_must_cover_the_rows():
    from matrixone_amd import engine
    c = bc.BY_NAME["n300"]
    ix = _index(c, "auto")
    try:
        Q = bc.inputs(c.name)[1]
        short = np.full(9, 0xFFFFFFFF, dtype=np.uint32)  # 288 bits < 300
        with pytest.raises(engine.MoannError, match="covers 288"):
            ix.search(Q, 10, row_bitset=short)
        ids, _ = ix.search(Q, 10, row_bitset=np.full(10, 0xFFFFFFFF,
                                                     dtype=np.uint32))
        assert (ids == bc.reference(c.name)[0]).all()
    finally:
        ix.close()


def test_delete_of_an_unknown_id_is_a_no_op():
    c = bc.BY_NAME["ids"]
    for mode in ("fused", "gemm"):
        ix = _index(c, mode)
        try:
            ix.delete(5)       # ids start at 1000
            ix.delete(-1)
            ids, dists = ix.search(bc.inputs(c.name)[1], c.k)
        finally:
            ix.close()
        bc.check_exact(c.name, ids, dists, f"unknown delete/{mode}")


@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("mode", ["fused", "gemm"])
def test_append_equals_a_fresh_index(mode, custom):
    """100 rows, a search, 200 more (the capacity of 128 grows to 512 on the
    way), a search: byte for byte what a fresh index over the 300 returns."""
    from matrixone_amd import engine
    X, Q, _ = bc.inputs("n300")
    ids = (5000 - 3 * np.arange(300, dtype=np.int64)) if custom else None
    cut = lambda a, lo, hi: None if a is None else a[lo:hi]

    def fresh(nrows):
        ix = engine.BruteForceIndex(64, capacity=nrows)
        ix.set_params(mode, 0)
        ix.add(X[:nrows], ids=cut(ids, 0, nrows))
        try:
            return ix.search(Q, 10)
        finally:
            ix.close()

    ix = engine.BruteForceIndex(64)
    try:
        ix.set_params(mode, 0)
        ix.add(X[:100], ids=cut(ids, 0, 100))
        first = ix.search(Q, 10)
        ix.add(X[100:], ids=cut(ids, 100, 300))
        assert len(ix) == 300
        second = ix.search(Q, 10)
    finally:
        ix.close()
    for got, want in ((first, fresh(100)), (second, fresh(300))):
        assert got[0].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes()
    ref = bc.reference("n300")[1]
    assert (second[0] == (ref if ids is None else ids[ref])).all()


def test_device_queries_and_perf():
    import torch
    c = bc.BY_NAME["n300"]
    ix = _index(c, "fused")
    try:
        Q = bc.inputs(c.name)[1]
        host = ix.search(Q, c.k)
        qd = torch.from_numpy(np.array(Q)).cuda()
        torch.cuda.synchronize()
        dev = ix.search_device(qd, c.k)
        assert host[0].tobytes() == dev[0].tobytes()
        assert host[1].tobytes() == dev[1].tobytes()
        p = ix.perf()
        assert p["scan_launches"] == 2 and p["scan_ms"] > 0
        assert p["scan_rows"] == 2 * c.n * c.nq
        empty = ix.search(Q[:0], c.k)  # nq = 0 returns at once
        assert empty[0].shape == (0, c.k)
    finally:
        ix.close()


def test_search_with_tail_takes_a_resident_tail():
    """search_with_tail(tail_index=...) equals the tail_vecs form. Integer
    coordinates: the one-shot entry's difference form and the resident
    index's expanded form then give the same f32 distances."""
    from matrixone_amd import engine
    rng = np.random.default_rng(12)
    X = rng.integers(-8, 9, (400, 16)).astype(np.float32)
    Q = rng.integers(-8, 9, (37, 16)).astype(np.float32)
    T = rng.integers(-8, 9, (50, 16)).astype(np.float32)
    t_ids = 10000 + np.arange(50, dtype=np.int64)
    C = X[:4].copy()
    assign = bc.dist_matrix(X, C, "l2sq").argmin(1).astype(np.int32)
    main = engine.IvfFlatIndex(16, 4, metric="l2sq", capacity=400)
    tail = engine.BruteForceIndex(16)
    try:
        main.add(X, ids=np.arange(400, dtype=np.int64))
        main.set_centroids(C)
        main.set_assignments(assign)
        main.build()
        tail.add(T[:20], ids=t_ids[:20])
        tail.add(T[20:], ids=t_ids[20:])
        want = engine.search_with_tail(main, Q, 10, 4, T, t_ids)
        got = engine.search_with_tail(main, Q, 10, 4, None, None,
                                      tail_index=tail)
        assert (want[0] >= 10000).any()  # the tail does reach the results
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        empty = engine.BruteForceIndex(16)
        only_main = engine.search_with_tail(main, Q, 10, 4, None, None,
                                            tail_index=empty)
        empty.close()
        np.testing.assert_array_equal(only_main[0], main.search(Q, 10, 4)[0])
    finally:
        main.close()
        tail.close()


def test_errors():
    from matrixone_amd import engine
    with pytest.raises(engine.MoannError, match="moann_brute_force_search"):
        engine.BruteForceIndex(8, metric="l1")
    X, Q, _ = bc.inputs("n300")
    ix = engine.BruteForceIndex(64)
    try:
        ix.add(X)
        with pytest.raises(engine.MoannError, match="dimension"):
            ix.search(Q[:, :63], 10)
        with pytest.raises(engine.MoannError, match=r"\[1, 4096\]"):
            ix.search(Q, 0)
        with pytest.raises(engine.MoannError, match=r"\[1, 4096\]"):
            ix.search(Q, 4097)
        with pytest.raises(engine.MoannError, match="multiple of the 128"):
            ix.set_params("auto", 100)
        with pytest.raises(engine.MoannError, match="mode"):
            ix.set_params(3, 0)
        ix.set_params("fused", 0)
        with pytest.raises(engine.MoannError, match="fused mode serves"):
            ix.search(Q, bc.KMAX + 1)
        ix.set_params("auto", 0)
        ids, _ = ix.search(Q, 4096)  # the largest k: 300 rows, then padding
        assert (ids[:, :300] >= 0).all() and (ids[:, 300:] == -1).all()
    finally:
        ix.close()
