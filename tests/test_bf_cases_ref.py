"""CPU self-test of the brute-force case table (tests/bf_cases.py): the
python-list restatement of the kernel must equal the f64 reference on every
exact case, each seeded corruption of it must be caught by its named case,
and no float case may have so many near-ties that the GPU test's excuse cap
could hide a wrong result. Also: the new C entries are in the built
library."""

import os
import subprocess

import numpy as np
import pytest

import bf_cases as bc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "matrixone_amd", "libmoann_hip.so")

EXACT_NAMES = [c.name for c in bc.EXACT]
FLOAT_NAMES = [c.name for c in bc.FLOAT]


def _model(name, corrupt=None):
    c = bc.BY_NAME[name]
    return bc.kernel_model(bc.dist64(name), bc.alive_and_filter_words(c),
                           c.k, bc.model_slice_rows(c), corrupt)


def _as_ids(name, rows):
    ids = bc.inputs(name)[2]
    return np.where(rows >= 0, ids[np.maximum(rows, 0)], -1)


def test_table_covers_the_edges():
    ex = bc.EXACT
    assert {c.n for c in ex} >= {1, 127, 128, 129, 300}
    assert {c.nq for c in ex} >= {1, 127, 129, 257}
    assert {c.dim for c in ex} >= {1, 3, 4, 33, 36, 64}
    assert {c.k for c in ex} >= {1, 10, bc.KMAX, bc.KMAX + 1}
    assert any(c.k > c.n for c in ex)
    assert all(c.dim <= 64 for c in ex)
    # the tie cases stay in launch_topk's position-ordered range
    for c in ex:
        slices = -(-c.n // (c.slice_rows or bc.TILE))
        assert slices * c.k <= 1024, c.name
    fl = bc.FLOAT
    assert {(c.n, c.dim) for c in fl} == {(1000, 100), (500, 33), (2000, 768)}
    assert {c.metric for c in fl} == {"l2sq", "l2", "ip", "cos"}
    assert all(c.nq == 64 for c in fl)


@pytest.mark.parametrize("name", EXACT_NAMES)
def test_model_equals_reference(name):
    rows, d = _model(name)
    ref_ids, ref_rows, ref_d = bc.reference(name)
    np.testing.assert_array_equal(rows, ref_rows)
    np.testing.assert_array_equal(d, ref_d)
    # and through the check the GPU result goes through
    bc.check_exact(name, _as_ids(name, rows), d.astype(np.float32), name)


@pytest.mark.parametrize("name", EXACT_NAMES)
def test_whole_tile_slicing_does_not_matter(name):
    """The planner may cut the rows into any whole-tile slices."""
    c = bc.BY_NAME[name]
    D, w = bc.dist64(name), bc.alive_and_filter_words(c)
    one = bc.kernel_model(D, w, c.k, 3 * bc.TILE)
    np.testing.assert_array_equal(one[0], bc.reference(name)[1])


@pytest.mark.parametrize("corrupt,name", sorted(bc.CORRUPTION_CASES.items()))
def test_corruption_is_caught(corrupt, name):
    rows, d = _model(name, corrupt)
    with pytest.raises(AssertionError):
        bc.check_exact(name, _as_ids(name, rows), d.astype(np.float32),
                       f"{name}/{corrupt}")


def test_expected_rows_of_the_tie_cases():
    """300 identical rows return rows 0..9; with bits cleared, the first
    surviving rows."""
    _, rows, _ = bc.reference("same300")
    assert (rows == np.arange(10)[None, :]).all()
    _, rows, _ = bc.reference("flt_edges")
    want = [r for r in range(300) if r not in (31, 32, 63, 64, 127, 128)]
    assert (rows == np.array(want[:bc.KMAX])[None, :]).all()
    ids, rows, d = bc.reference("flt_all")
    assert (ids == -1).all() and (d == bc.F32_MAX).all()
    ids, _, _ = bc.reference("flt_few")
    assert ((ids >= 0).sum(1) == 5).all()


@pytest.mark.parametrize("name", FLOAT_NAMES)
def test_float_case_has_few_near_ties(name):
    count, ranks = bc.near_tie_ranks(name)
    print(f"{name}: {count} near-tie ranks of {ranks}")
    assert count < bc.NEAR_TIE_CAP * ranks, (name, count, ranks)


@pytest.mark.parametrize("name", ["mix500x33_l2sq", "mix500x33_cos",
                                  "mix500x33_l2", "mix500x33_ip"])
def test_float_check_accepts_f32_and_rejects_defects(name):
    """check_float on an honest f32 evaluation of the expanded form, and on
    three defects: a shifted result, a repeated id, a distance off by 10x
    its bound."""
    c = bc.BY_NAME[name]
    X, Q, ids = bc.inputs(name)
    m = "l2sq" if c.metric == "l2" else c.metric
    D32 = bc.dist_matrix(Q, X, m, np.float32)
    if c.metric == "l2":
        D32 = np.sqrt(D32.astype(np.float64)).astype(np.float32)
    got_i, got_r, got_d = bc.topk_of(D32, bc.allowed_mask(c), ids, c.k)
    got_d = got_d.astype(np.float32)
    bc.check_float(name, got_i, got_d, name)
    q = 5
    with pytest.raises(AssertionError):  # rank 0 dropped
        bad_i, bad_d = got_i.copy(), got_d.copy()
        ri, _, rd = bc.topk_of(D32, bc.allowed_mask(c), ids, c.k + 1)
        bad_i[q], bad_d[q] = ri[q, 1:], rd[q, 1:]
        bc.check_float(name, bad_i, bad_d, name)
    with pytest.raises(AssertionError, match="repeated id"):
        bad_i = got_i.copy()
        bad_i[q, 1] = bad_i[q, 0]
        bc.check_float(name, bad_i, got_d, name)
    with pytest.raises(AssertionError, match="distance"):
        bad_d = got_d.copy()
        row = int(got_r[q, 2])
        bad_d[q, 2] += np.float32(10 * bc.dist_tol(X, Q, c.metric)[q, row])
        bc.check_float(name, got_i, bad_d, name)


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True,
                         capture_output=True, text=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if line.strip()}
    want = {"moann_bf_new", "moann_bf_add", "moann_bf_delete_id",
            "moann_bf_set_params", "moann_bf_search", "moann_bf_search_device",
            "moann_bf_search_filtered", "moann_bf_len", "moann_bf_fused_kmax",
            "moann_bf_perf", "moann_bf_destroy"}
    assert want <= have, sorted(want - have)
    assert "moann_brute_force_search" in have  # the one-shot entry stays
