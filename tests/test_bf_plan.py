"""CPU check of the brute-force planner (matrixone_amd/csrc/moann_bf_plan.h).

How a search of the resident brute-force index is cut into query batches,
row slices and buffers, and how its row store grows, is pure integer code;
bf_plan_check.cpp asserts the invariants at the tile, slice and size edges.
It is a stand-alone host program built with ASan + UBSan
(`make bf_plan_check`), run here as a child process."""

import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "matrixone_amd", "csrc")


def test_bf_plan_check_passes_under_sanitizers():
    subprocess.run(["make", "-s", "bf_plan_check"], cwd=CSRC, check=True)
    r = subprocess.run([os.path.join(CSRC, "bf_plan_check")],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("bf_plan_check OK"), r.stdout
