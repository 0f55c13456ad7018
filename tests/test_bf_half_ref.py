"""CPU self-test of the f16 brute-force case table (tests/bf_half_cases.py):
the new exact cases really are exact in binary16 and in f32, the python-list
restatement of the kernel equals their reference, the seeded corruptions are
still caught at a dim that crosses a slab, and on the ROUNDED inputs no float
case has so many near-ties that the GPU test's excuse cap could hide a wrong
result. Also: the new C entries are in the built library, and the planner
check (extended for the widened gemm tile) passes under its sanitizers."""

import os
import subprocess

import numpy as np
import pytest

import bf_cases as bc
import bf_half_cases as hc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "matrixone_amd", "libmoann_hip.so")
CSRC = os.path.join(REPO, "matrixone_amd", "csrc")

NEW_NAMES = [c.name for c in hc.NEW]

# near-tie ranks of the reference on the rounded inputs (count, ranks)
NEAR_TIES = {
    "mix1000x100_l2sq": (0, 640), "mix1000x100_l2": (0, 640),
    "mix1000x100_ip": (0, 640), "mix1000x100_cos": (1, 630),
    "mix500x33_l2sq": (0, 640), "mix500x33_l2": (0, 640),
    "mix500x33_ip": (0, 640), "mix500x33_cos": (1, 630),
    "mix2000x768_l2sq": (1, 640), "mix2000x768_l2": (4, 640),
    "mix2000x768_ip": (0, 640), "mix2000x768_cos": (0, 630),
    "mix500x33_kmax": (15, 4096), "mix500x33_kbig": (27, 4160),
    "mix500x33_slices": (0, 640),
}


def _model(c, corrupt=None):
    return bc.kernel_model(hc.dist64(c.name), bc.alive_and_filter_words(c),
                           c.k, bc.model_slice_rows(c), corrupt)


def test_table_covers_the_f16_edges():
    new = hc.NEW_EXACT
    assert {c.dim for c in new} >= {7, 8, 33, 65, 72, 127, 129, 200}
    assert {c.metric for c in new} == {"l2sq", "ip", "l2"}
    assert {c.k for c in new} >= {1, 10, bc.KMAX, bc.KMAX + 1}
    assert any(c.kind == "quarter" for c in new)
    assert all(c in hc.EXACT for c in bc.EXACT)  # the old cases, unchanged
    assert hc.FLOAT == bc.FLOAT
    for c in hc.NEW:  # the tie cases stay in launch_topk's ordered range
        slices = -(-c.n // (c.slice_rows or bc.TILE))
        assert slices * c.k <= 1024, c.name


@pytest.mark.parametrize("name", [c.name for c in hc.EXACT])
def test_exact_cases_are_exact_in_f16_and_f32(name):
    """The rounding changes nothing, and every norm, dot product and distance
    is an integer below 2^24 (the quarter case in units of 1/16), so every
    f32 operation on them is exact in any order."""
    c = hc.BY_NAME[name]
    X, Q, _ = hc.inputs(name)
    Xh, Qh, _ = hc.stored(name)
    assert (Xh == X).all() and (Qh == Q).all()
    s = 4.0 if c.kind == "quarter" else 1.0
    X64, Q64 = X.astype(np.float64) * s, Q.astype(np.float64) * s
    assert (X64 == np.rint(X64)).all() and (Q64 == np.rint(Q64)).all()
    norms = max((X64 ** 2).sum(1).max(), (Q64 ** 2).sum(1).max())
    dots = (np.abs(Q64) @ np.abs(X64).T).max()  # bounds every partial sum
    dist = hc.dist_matrix(Q64, X64, "l2sq").max()
    print(f"{name}: norm {norms:.0f} |dot| {dots:.0f} l2sq {dist:.0f}")
    # qn + xn - 2 dot, whatever the order of its three terms
    assert max(dist, 2 * norms + 2 * dots) < 2.0 ** 24


def test_dim_200_magnitudes():
    """The figures the case table rests on."""
    X, Q, _ = hc.inputs("h_d200_kmax")
    n = max((X.astype(np.float64) ** 2).sum(1).max(),
            (Q.astype(np.float64) ** 2).sum(1).max())
    d = hc.dist_matrix(Q, X, "l2sq").max()
    assert n <= 200 * 64 and d <= 200 * 256
    assert n < 2 ** 14 and d < 2 ** 16


@pytest.mark.parametrize("name", NEW_NAMES)
def test_model_equals_reference(name):
    c = hc.BY_NAME[name]
    rows, d = _model(c)
    ref_ids, ref_rows, ref_d = hc.reference(name)
    np.testing.assert_array_equal(rows, ref_rows)
    np.testing.assert_array_equal(d, ref_d)
    hc.check_exact(name, rows, d.astype(np.float32), name)  # ids == rows


@pytest.mark.parametrize("name", [c.name for c in bc.EXACT])
def test_old_exact_cases_keep_their_reference(name):
    a, b = hc.reference(name), bc.reference(name)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("corrupt", sorted(hc.CORRUPTION_CASES))
def test_corruption_is_caught_at_dim_65(corrupt):
    c = hc.CORRUPTION_CASES[corrupt]
    assert c.dim == 65
    rows, d = _model(c, corrupt)
    with pytest.raises(AssertionError):
        hc.check_exact(c.name, rows, d.astype(np.float32),
                       f"{c.name}/{corrupt}")


@pytest.mark.parametrize("name", [c.name for c in hc.FLOAT])
def test_float_case_has_few_near_ties_on_rounded_inputs(name):
    Xh, Qh, _ = hc.stored(name)
    assert np.isfinite(Xh).all() and np.isfinite(Qh).all()
    count, ranks = hc.near_tie_ranks(name)
    print(f"{name}: {count} near-tie ranks of {ranks}")
    assert count <= hc.NEAR_TIE_CAP * ranks, (name, count, ranks)
    assert (count, ranks) == NEAR_TIES[name]


def test_float_check_accepts_f32_and_rejects_defects():
    """hc.check_float on an honest f32 evaluation over the rounded inputs,
    and on a dropped rank, a repeated id and a distance 10x off its bound."""
    name = "mix500x33_l2sq"
    c = hc.BY_NAME[name]
    Xh, Qh, ids = hc.stored(name)
    D32 = hc.dist_matrix(Qh, Xh, "l2sq", np.float32)
    got_i, got_r, got_d = hc.topk_of(D32, bc.allowed_mask(c), ids, c.k)
    got_d = got_d.astype(np.float32)
    hc.check_float(name, got_i, got_d, name)
    q = 5
    with pytest.raises(AssertionError):
        bad_i, bad_d = got_i.copy(), got_d.copy()
        ri, _, rd = hc.topk_of(D32, bc.allowed_mask(c), ids, c.k + 1)
        bad_i[q], bad_d[q] = ri[q, 1:], rd[q, 1:]
        hc.check_float(name, bad_i, bad_d, name)
    with pytest.raises(AssertionError, match="repeated id"):
        bad_i = got_i.copy()
        bad_i[q, 1] = bad_i[q, 0]
        hc.check_float(name, bad_i, got_d, name)
    with pytest.raises(AssertionError, match="distance"):
        bad_d = got_d.copy()
        bad_d[q, 2] += np.float32(10 * hc.tol(name)[q, int(got_r[q, 2])])
        hc.check_float(name, got_i, bad_d, name)
    # the unrounded reference is a different question: bf_cases' own check
    # over the same result must notice (the inputs move by up to 2^-11)
    with pytest.raises(AssertionError):
        bc.check_float(name, got_i, got_d, name)


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True,
                         capture_output=True, text=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if line.strip()}
    want = {"moann_bf_new_typed", "moann_bf_add_half", "moann_bf_storage"}
    assert want <= have, sorted(want - have)


def test_bf_plan_check_covers_the_widened_tile():
    subprocess.run(["make", "-s", "bf_plan_check"], cwd=CSRC, check=True)
    r = subprocess.run([os.path.join(CSRC, "bf_plan_check")],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("bf_plan_check OK"), r.stdout
    src = open(os.path.join(CSRC, "bf_plan_check.cpp")).read()
    assert "check_wide_plan" in src and "BF_WIDE_CAP" in src
