"""CPU self-test of tests/select_cases.py: the conditions that make the
GPU comparison of tests/test_select_gpu.py honest hold for every case, and
the steered rows do to the filter's rule what their names say."""

import numpy as np
import pytest

import select_cases as sc


@pytest.mark.parametrize("name", sc.names())
def test_no_value_repeats_past_the_radix_tie_mode(name):
    """More than 1024 equal values at the cut would end the radix select in
    its level-3 tie mode, where atomic order picks the ids; the cases stay
    far below: no value occurs more than MAX_REPEAT times in a row."""
    c = sc.cases()[name]
    for q in range(c.nq):
        if c.row(q).size:
            _, n = np.unique(sc.f2u(c.row(q)), return_counts=True)
            assert n.max() <= sc.MAX_REPEAT, (name, q, int(n.max()))


@pytest.mark.parametrize("name", sc.names())
def test_reference_is_the_k_smallest(name):
    """The reference against a plain stable argsort of the values, on rows
    where value order and key order agree (no -0.0, no NaN)."""
    c = sc.cases()[name]
    slots, dists = sc.reference(name)
    assert slots.shape == dists.shape == (c.nq, c.k)
    for q in range(c.nq):
        r = c.row(q)
        m = min(c.k, r.size)
        assert (slots[q, m:] == -1).all() and (dists[q, m:] == sc.FLT_MAX).all()
        assert (np.diff(sc.f2u(dists[q, :m]).astype(np.int64)) >= 0).all()
        if not (np.signbit(r) & (r == 0)).any():
            np.testing.assert_array_equal(
                slots[q, :m], np.argsort(r, kind="stable")[:m])


def test_ragged_rows_cover_every_alignment():
    """Among the rows that take the filter path every off % 4 (the scalar
    head is (4 - off % 4) % 4 long) and every scalar tail length occurs."""
    c = sc.cases()["ragged-k64"]
    M = sc.constants()["MIN"]
    counts = np.diff(c.qoffs)
    assert counts.tolist() == [1001, M - 1, M, M + 1, M + 2, M + 3, M + 17,
                               3 * M + 5]
    assert sc.simulate(c.row(1), c.k) is None      # M - 1: straight to radix
    heads, tails = set(), set()
    for q in range(2, c.nq):
        assert sc.simulate(c.row(q), c.k) is not None
        head = int(-c.qoffs[q] % 4)
        heads.add(head)
        tails.add(int((counts[q] - head) % 4))
    assert heads == tails == {0, 1, 2, 3}


def test_engage_limits():
    c = sc.constants()
    M, KMAX = c["MIN"], c["KMAX"]
    assert sc.plan(M, 64)["filter"] and not sc.plan(M - 1, 64)["filter"]
    assert sc.plan(M, KMAX)["filter"] and not sc.plan(M, KMAX + 1)["filter"]
    big = sc.cases()["ragged-kmax+1"]
    assert big.k == KMAX + 1 and sc.cases()["ragged-kmax"].k == KMAX
    assert sorted(sc.cases()) == sorted(sc.NAMES)
    assert all(sc.simulate(big.row(q), big.k) is None for q in range(big.nq))


def test_special_rows():
    c = sc.cases()["special"]
    slots, dists = sc.reference("special")
    top = dists[1]
    assert (top[:5] < 0).all()
    assert (np.signbit(top[5:25]) & (top[5:25] == 0)).all()     # -0.0 first
    assert (~np.signbit(top[25:45]) & (top[25:45] == 0)).all()  # then +0.0
    assert (top[45:] > 0).all() and (top < sc.FLT_MAX).all()
    assert sc.simulate(c.row(1), c.k) is not None
    short = c.row(2)
    assert (short < sc.FLT_MAX).sum() < c.k
    assert (dists[2, 30:] == sc.FLT_MAX).all() and (slots[2] >= 0).all()


def test_steered_rows_fall_back_and_the_gaussian_does_not():
    cap = sc.constants()["CAP"]
    u = sc.cases()["undershoot"]
    got, fb = sc.simulate(u.row(1), u.k)
    assert fb and got == sc.plan(u.row(1).size, u.k)["rank"] < u.k
    o = sc.cases()["overflow"]
    got, fb = sc.simulate(o.row(1), o.k)
    assert fb and got > cap
    assert sc.expected_fallbacks("undershoot") == 1
    assert sc.expected_fallbacks("overflow") == 1
    g = sc.cases()["gauss20000"]
    got, fb = sc.simulate(g.row(0), g.k)
    assert not fb and g.k <= got <= cap
    assert sc.expected_fallbacks("gauss20000") == 0
