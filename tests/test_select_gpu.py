"""The two ragged selection kernels through moann_select_topk: the radix
select (mode 0) and the threshold filter with its radix fallback (mode 1)
against the numpy definition in tests/select_cases.py — slots and distance
bits, exactly — and the filter's fallback count against the rule applied on
the CPU.

Paths of select_filter_kernel reached: rows below the engage count and k
above the filter's limit (straight to the radix function), every off % 4 and
scalar tail length, one to several float4 rounds, the sort of 64..2048
collected keys, the undershoot and the overflow fallback."""

import numpy as np
import pytest

import select_cases as sc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sc.names())
def test_filter_equals_radix_equals_reference(name):
    from matrixone_amd import engine
    c = sc.cases()[name]
    ref_s, ref_d = sc.reference(name)
    s0, d0, fb0, _ = engine.select_topk(c.dists, c.qoffs, c.k, "radix")
    s1, d1, fb1, _ = engine.select_topk(c.dists, c.qoffs, c.k, "filter")
    print(f"{name}: fallbacks {fb1}, expected {sc.expected_fallbacks(name)}")
    np.testing.assert_array_equal(s0, ref_s, err_msg=f"{name} radix slots")
    np.testing.assert_array_equal(_bits(d0), _bits(ref_d),
                                  err_msg=f"{name} radix dists")
    np.testing.assert_array_equal(s1, ref_s, err_msg=f"{name} filter slots")
    np.testing.assert_array_equal(_bits(d1), _bits(ref_d),
                                  err_msg=f"{name} filter dists")
    assert fb0 == 0
    assert fb1 == sc.expected_fallbacks(name)


def test_fallback_counts():
    """The steered rows are counted as fallen back, a plain Gaussian row of
    20 000 is not."""
    from matrixone_amd import engine
    for name, want in (("undershoot", 1), ("overflow", 1), ("gauss20000", 0)):
        c = sc.cases()[name]
        assert sc.expected_fallbacks(name) == want
        _, _, fb, _ = engine.select_topk(c.dists, c.qoffs, c.k, "filter")
        assert fb == want, name
