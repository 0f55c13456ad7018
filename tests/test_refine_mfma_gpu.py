"""The MFMA byte scan of the refine path against the CPU reference in
oracle/refine.py and against the dot kernel, on the cases of
tests/refine_mfma_cases.py. As in tests/test_refine_gpu.py every search runs
first on a fresh index.

Kernel reached by each case (signed refine image, QT = 16, dpad % 64 == 0,
so the image is MFMA-ordered and launch_scan_i8 takes the MFMA kernel):
  mf-{l2sq,ip,cos}-d128-R*   scan_i8_mfma_kernel<L2SQ|IP|COS>, 2 K-steps
  mf-{l2sq,ip,cos}-d192-R*   scan_i8_mfma_kernel<L2SQ|IP|COS>, 3 K-steps
  mf-tile-{ip,cos}-nq*       scan_i8_mfma_kernel<IP|COS>, 1 K-step; tiles of
                             1, 15, 16, 16+1 and 16+16+1 queries
  mf-filt-rate30             scan_i8_mfma_kernel<L2SQ> with the filter bitset
  A/B, default child         scan_i8_mfma_kernel<L2SQ>, 1 and 2 K-steps
  A/B, MOANN_BYTE_MFMA=0     scan_i8_dot_kernel<L2SQ, false, 16> over the
                             row-ordered image
The lists of refine_cases.SIZES give jobs of 8, 4, 3, 2 and 1 groups, so a
wave streams 2, 1 or 0 groups: 1 to 6 steps of 4 KiB here, which is the ring
prologue and the peeled tail with fewer steps than ring slots, exactly as
many, and more; the steady-state loop runs at d = 192 (6 steps) and in the
d = 768 cases of tests/test_refine_gpu.py (12 and 24 steps)."""

import os
import subprocess
import sys

import numpy as np
import pytest

import refine_cases as rc
import refine_mfma_cases as mc
from oracle import refine as rf

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))


def _names(prefix):
    return [c.name for c in mc.CASES if c.name.startswith(prefix)]


def _fresh_index(c):
    from matrixone_amd import engine
    cp = rc.corpus(c.kind, c.d)
    ix = engine.IvfFlatIndex(c.d, rc.NLIST, metric=c.metric,
                             capacity=cp.vecs.shape[0])
    ix.add(cp.vecs, ids=cp.ids)
    ix.set_centroids(cp.cents)
    ix.set_assignments(cp.assign.astype(np.int32))
    ix.build()
    return ix


def _check(c, ids, dists, allowed=None, ctx=""):
    skipped, n_must = rf.check_two_stage(
        ids, dists, rc.reference(c), c.k, c.R, allowed=allowed,
        ctx=f"{c.name}{ctx}")
    print(f"{c.name}{ctx}: skipped {skipped} of {n_must} must candidates")
    assert skipped <= rc.SKIP_CAP * n_must, (c.name, skipped, n_must)


def _assert_exact_parity(c, ids, dists):
    """R >= every candidate count: the result must equal the plain exact
    search of the oracle (ids bit-exact except at FP ties)."""
    from test_parity_gpu import _assert_parity
    cp = rc.corpus(c.kind, c.d)
    om, orig_l2 = rc.METRICS[c.metric]
    ref_ids, ref_d = cp.idx.search(om, rc.queries(c), c.probe, c.k,
                                   orig_l2=orig_l2)
    np.testing.assert_array_equal(ids == -1, ref_ids == -1, err_msg=c.name)
    _assert_parity(ids, dists, ref_ids, ref_d, ctx=c.name)


def _run_case(c):
    ix = _fresh_index(c)
    try:
        ix.enable_refine(c.depth)
        ids, dists = ix.search(rc.queries(c), c.k, c.probe)
    finally:
        ix.close()
    if c.depth >= 4096:
        _assert_exact_parity(c, ids, dists)
    _check(c, ids, dists)


@pytest.mark.parametrize("name", _names("mf-l2sq-") + _names("mf-ip-") +
                         _names("mf-cos-"))
def test_k_steps_and_metrics(name):
    """2 and 3 K-steps of 64 dims for every metric the kernel has; at full
    depth the result is the exact search, at depth 32 the band contract."""
    _run_case(mc.BY_NAME[name])


@pytest.mark.parametrize("name", _names("mf-tile-"))
def test_tile_tails_ip_cos(name):
    """probe = nlist, so nq sets the tile shapes: one query, one short of a
    tile, a full tile, one and two tiles plus one."""
    _run_case(mc.BY_NAME[name])


def test_filtered():
    c = mc.BY_NAME["mf-filt-rate30"]
    cp = rc.corpus(c.kind, c.d)
    allowed = rc.allowed_rows(c)
    ix = _fresh_index(c)
    try:
        ix.enable_refine(c.depth)
        ids, dists = ix.search_filtered(rc.queries(c), c.k, c.probe,
                                        ix.filter_bitset(cp.ids[allowed]))
    finally:
        ix.close()
    _check(c, ids, dists, allowed=allowed)


def test_clip_bounds_reach_the_scan():
    for d in sorted({c.d for c in mc.CASES}):
        codes = rc.corpus("std", d).codes
        assert (codes == -128).any() and (codes == 127).any(), d


def _child(tmp_path, tag, mfma_off):
    out = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ)
    env.pop("MOANN_BYTE_MFMA", None)
    if mfma_off:
        env["MOANN_BYTE_MFMA"] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    cmd += [os.path.join(TESTS, "refine_mfma_child.py"), out]
    cmd += [c.name for c in mc.AB_CASES]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
    return np.load(out)


def test_ab_against_dot_kernel(tmp_path):
    """The same l2sq searches (1 and 2 K-steps) in a fresh process per
    kernel: distances equal bit for bit, ids equal wherever a query's
    returned distances are distinct; both meet the reference contract."""
    new = _child(tmp_path, "mfma", mfma_off=False)
    old = _child(tmp_path, "dot", mfma_off=True)
    for c in mc.AB_CASES:
        d_new, d_old = new[c.name + ":dists"], old[c.name + ":dists"]
        i_new, i_old = new[c.name + ":ids"], old[c.name + ":ids"]
        assert d_new.dtype == d_old.dtype == np.float32
        np.testing.assert_array_equal(d_new.view(np.uint32),
                                      d_old.view(np.uint32), err_msg=c.name)
        for q in range(c.nq):
            if np.unique(d_new[q]).size == d_new[q].size:
                np.testing.assert_array_equal(i_new[q], i_old[q],
                                              err_msg=f"{c.name} q{q}")
        _check(c, i_new, d_new, ctx=" mfma child")
        _check(c, i_old, d_old, ctx=" dot child")
