"""CPU side of tests/test_refine_mfma_gpu.py: on the inputs of every case in
tests/refine_mfma_cases.py the ideal two-stage result passes the tie-tolerant
contract of oracle/refine.py within the skip cap, so the cap the GPU test
asserts is a condition the reference itself meets on these shapes."""

import pytest

import refine_cases as rc
import refine_mfma_cases as mc
from oracle import refine as rf


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_ideal_passes_and_skip_cap(name):
    c = mc.BY_NAME[name]
    ref = rc.reference(c)
    allowed = rc.allowed_rows(c)
    ids, d = rf.ideal_two_stage(ref, c.k, c.R, allowed=allowed)
    skipped, n_must = rf.check_two_stage(ids, d, ref, c.k, c.R,
                                         allowed=allowed, ctx=name)
    print(f"{name}: skipped {skipped} of {n_must} must candidates")
    assert n_must > 0
    assert skipped <= rc.SKIP_CAP * n_must, (name, skipped, n_must)


def test_clip_bounds_in_codes():
    """Both clip bounds occur in the byte image of every dim these cases
    use, so -128 and 127 go through the MFMA."""
    for d in sorted({c.d for c in mc.CASES}):
        codes = rc.corpus("std", d).codes
        assert (codes == -128).any() and (codes == 127).any(), d
