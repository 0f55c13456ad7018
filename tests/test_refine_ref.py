"""CPU self-test of the two-stage refine reference (oracle/refine.py), on
the inputs of every GPU case in tests/refine_cases.py: the ideal result must
pass the tie-tolerant contract, and each seeded corruption must be rejected
by the clause that owns it — so the GPU tests cannot pass vacuously."""

import numpy as np
import pytest

import refine_cases as rc
from oracle import oracle as orc
from oracle import refine as rf


def _ideal(c):
    ref = rc.reference(c)
    allowed = rc.allowed_rows(c)
    ids, d = rf.ideal_two_stage(ref, c.k, c.R, allowed=allowed)
    return ref, allowed, ids, d


def _positions(ref, qi, ids):
    """candidate positions of returned ids"""
    cand_ids = ref.row_ids[ref.cand_rows[qi]]
    lut = {int(v): i for i, v in enumerate(cand_ids)}
    return np.array([lut[int(i)] for i in ids if i >= 0], dtype=np.int64)


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_ideal_passes_and_skip_cap(name):
    c = rc.BY_NAME[name]
    ref, allowed, ids, d = _ideal(c)
    skipped, n_must = rf.check_two_stage(ids, d, ref, c.k, c.R,
                                         allowed=allowed, ctx=name)
    assert skipped <= rc.SKIP_CAP * n_must, (name, skipped, n_must)


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_corruptions_rejected(name):
    c = rc.BY_NAME[name]
    ref, allowed, ids, d = _ideal(c)
    k, R = c.k, c.R
    cos = ref.metric == orc.METRIC_COS

    def rejects(bad_ids, bad_d, qi, clause, mask=allowed):
        with pytest.raises(AssertionError, match=clause):
            rf.check_two_stage(bad_ids, bad_d, ref, k, R, allowed=mask,
                               ctx=name, only=[qi])

    # 1. stage 1 drops a MUST candidate and keeps one from outside MAY
    #    instead (tile lanes 8..15 holding stale values): the best returned
    #    candidate that stage 1 had to keep goes missing.
    done = False
    for qi in range(ref.nq):
        pm = rf._pass_mask(ref, qi, allowed)
        must, may = rf.stage1_band(ref.bdist[qi], pm, R, cos=cos)
        pos = _positions(ref, qi, ids[qi])
        hit = [p for p in pos if must[p]]
        if not hit:
            continue
        outside = np.flatnonzero(pm & ~may)
        add = int(outside[0]) if outside.size else None
        bi, bd = rf.ideal_two_stage(ref, k, R, allowed=allowed,
                                    stage1_edit=(qi, int(hit[0]), add))
        rejects(bi, bd, qi, r"\((a|d|e)\)")
        done = True
        break
    assert done, "case has no query with a MUST candidate in its result"

    # 2. one returned distance off by 1e-4 relative
    live = ids >= 0
    qi, j = np.unravel_index(np.argmax(np.where(live, np.abs(d), -1.0)),
                             d.shape)
    bd = d.copy()
    bd[qi, j] = np.float32(float(d[qi, j]) * (1.0 + 1e-4))
    rejects(ids, bd, qi, r"\((b|c)\)")

    # 3a. two entries of one output row swapped
    done = False
    for qi in range(ref.nq):
        n = int(live[qi].sum())
        if n >= 2 and d[qi, 0] != d[qi, n - 1]:
            bi, bd = ids.copy(), d.copy()
            bi[qi, [0, n - 1]] = ids[qi, [n - 1, 0]]
            bd[qi, [0, n - 1]] = d[qi, [n - 1, 0]]
            rejects(bi, bd, qi, r"\(c\)")
            done = True
            break
    assert done or k == 1
    # 3b. the output rows of two queries swapped
    if ref.nq >= 2:
        q0 = next(q for q in range(ref.nq) if live[q].any())
        q1 = next(q for q in range(ref.nq)
                  if q != q0 and not np.array_equal(ids[q], ids[q0]))
        bi, bd = ids.copy(), d.copy()
        bi[[q0, q1]] = ids[[q1, q0]]
        bd[[q0, q1]] = d[[q1, q0]]
        rejects(bi, bd, q0, r"\((a|b|d|e)\)")

    # 4. a filtered-out id returned: the result is judged under a filter
    #    that excludes one of its ids ...
    npass = [int(rf._pass_mask(ref, q, allowed).sum())
             for q in range(ref.nq)]
    qi = int(np.argmax(npass))
    assert npass[qi] > min(k, R), "no query keeps its count under the filter"
    base = (np.ones(ref.row_ids.size, dtype=bool) if allowed is None
            else allowed)
    rejects(ids, d, qi, r"\(a\).*filtered-out",
            mask=base & (ref.row_ids != ids[qi, 0]))
    # ... and, where the case has a filter, a rejected candidate is put into
    # the result at its exact distance
    if allowed is not None:
        for qi in range(ref.nq):
            pm = rf._pass_mask(ref, qi, allowed)
            n = int(live[qi].sum())
            if n and (~pm).any():
                p = int(np.flatnonzero(~pm)[0])
                bi, bd = ids.copy(), d.copy()
                bi[qi, n - 1] = ref.row_ids[ref.cand_rows[qi][p]]
                bd[qi, n - 1] = ref.exact[qi][p]
                o = np.argsort(bd[qi, :n], kind="stable")
                bi[qi, :n], bd[qi, :n] = bi[qi, :n][o], bd[qi, :n][o]
                rejects(bi, bd, qi, r"\(a\).*filtered-out")
                break

    # 5. a live entry replaced by padding
    qi = next(q for q in range(ref.nq) if live[q].any())
    n = int(live[qi].sum())
    bi, bd = ids.copy(), d.copy()
    bi[qi, n - 1] = -1
    bd[qi, n - 1] = rf.FLT_MAX
    rejects(bi, bd, qi, r"\(d\)")


def test_rq_params_and_quantize_match_f64_restatement():
    """The clip quantizer on an array whose quantiles, .5 rounding points
    and out-of-range values are all exact in f32 and f64 alike."""
    # 2000 values -> nlo = 2: two values below lo and two above hi
    body = np.concatenate([
        np.arange(-127, 128, dtype=np.float64),          # land on x.5
        np.arange(-127, 127, dtype=np.float64) + 0.5,    # land on integers
    ])
    body = np.resize(body, 2000 - 6)
    x = np.concatenate([[-1000.0, -300.0, -127.5], body,
                        [127.5, 200.0, 1000.0]]).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.permutation(x).reshape(250, 8)
    mul, add = rf.rq_params(x)
    # direct f64 restatement
    flat = np.sort(x.astype(np.float64).reshape(-1))
    nlo = flat.size // 1000
    lo, hi = flat[nlo], flat[flat.size - 1 - nlo]
    assert (lo, hi) == (-127.5, 127.5)
    assert float(mul) == 255.0 / (hi - lo) == 1.0
    assert float(add) == -lo * (255.0 / (hi - lo)) - 128.0 == -0.5
    s = x.astype(np.float64) * float(mul) + float(add)
    want = np.clip(np.copysign(np.floor(np.abs(s) + 0.5), s), -128, 127)
    got = rf.rq_quantize(x, mul, add)
    assert got.dtype == np.int8
    np.testing.assert_array_equal(got.astype(np.int64), want.astype(np.int64))
    # the interesting points really are in there
    assert (np.abs(s - np.trunc(s)) == 0.5).sum() > 200   # ties
    assert (s > 127.5).any() and (s < -128.5).any()       # clipped
    # ties go away from zero on both sides; clip saturates
    one = lambda v: int(rf.rq_quantize(np.float32([v]), mul, add)[0])
    assert one(3.0) == 3 and one(-2.0) == -3      # 2.5 -> 3, -2.5 -> -3
    assert one(1000.0) == 127 and one(-1000.0) == -128

    # general inputs: parameters equal the f64 formula cast to f32
    v = rng.standard_normal((500, 24), dtype=np.float32)
    mul, add = rf.rq_params(v)
    flat = np.sort(v.astype(np.float64).reshape(-1))
    nlo = flat.size // 1000
    lo, hi = flat[nlo], flat[flat.size - 1 - nlo]
    assert mul == np.float32(255.0 / (hi - lo))
    assert add == np.float32(-lo * (255.0 / (hi - lo)) - 128.0)
    # and the codes are within one step of the single-rounding f64 value,
    # equal wherever that value is not within f32 rounding of a .5 point
    s = v.astype(np.float64) * float(mul) + float(add)
    want = np.clip(np.copysign(np.floor(np.abs(s) + 0.5), s), -128, 127)
    got = rf.rq_quantize(v, mul, add).astype(np.float64)
    near_tie = np.abs(np.abs(s - np.floor(s)) - 0.5) < 1e-4
    np.testing.assert_array_equal(got[~near_tie], want[~near_tie])
    assert np.abs(got - want).max() <= 1


def test_byte_dists_cast_and_band():
    """byte_dists applies the kernel's float cast; stage1_band splits a tie
    group at T into MAY-only and keeps everything when <= R pass."""
    codes = np.array([[127] * 4096, [-128] * 4096], dtype=np.int8)
    q = np.array([-128] * 4096, dtype=np.int8)
    b = rf.byte_dists(orc.METRIC_L2SQ, codes, q)
    assert b.dtype == np.float32
    assert b[0] == np.float32(255 * 255 * 4096) and b[1] == 0
    b = np.float32([5, 1, 3, 3, 3, 9, 2])
    pm = np.array([1, 1, 1, 1, 1, 1, 0], dtype=bool)
    must, may = rf.stage1_band(b, pm, 3)
    assert must.tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert may.tolist() == [0, 1, 1, 1, 1, 0, 0]
    must, may = rf.stage1_band(b, pm, 6)
    assert must.tolist() == may.tolist() == pm.tolist()
