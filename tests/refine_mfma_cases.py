"""Cases for the MFMA byte scan of the refine path (scan_i8_mfma_kernel over
the MFMA-ordered refine image), shared by tests/test_refine_mfma_ref.py (CPU)
and tests/test_refine_mfma_gpu.py. They add to tests/refine_cases.py, whose
corpora, queries and cached references they reuse, the shapes that table
does not reach: 2 and 3 K-steps of 64 dims, IP and COS tile tails at one
K-step, and a filter at two K-steps."""

import refine_cases as rc


def _table():
    t = []
    # 2 and 3 K-steps x metric x depth (4096 == exact search)
    for d in (128, 192):
        for metric in ("l2sq", "ip", "cos"):
            for depth in (32, 4096):
                t.append(rc.Case(f"mf-{metric}-d{d}-R{depth}", d, metric, 25,
                                 depth=depth))
    # tile tails for the metrics whose finish differs from L2 (one K-step)
    for metric in ("ip", "cos"):
        for nq in (1, 15, 16, 17, 33):
            t.append(rc.Case(f"mf-tile-{metric}-nq{nq}", 64, metric, nq))
    # per-row filter at two K-steps
    t.append(rc.Case("mf-filt-rate30", 128, "l2sq", 25, filt="rate30"))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert not set(BY_NAME) & set(rc.BY_NAME)

# the l2sq cases run once per kernel in child processes (MOANN_BYTE_MFMA is
# read once per process): one K-step from the shared table, two from this one
AB_CASES = (rc.BY_NAME["tile-d64-nq25"], BY_NAME["mf-l2sq-d128-R32"])


def lookup(name):
    return BY_NAME[name] if name in BY_NAME else rc.BY_NAME[name]
