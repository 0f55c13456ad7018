"""CPU check of the threshold-filter selection's rule
(matrixone_amd/csrc/moann_select_plan.h).

Which rows take the filter path, where the sample is read and which sample
rank becomes the threshold is pure integer code; select_plan_check.cpp
asserts its invariants at the engage count, the k limit and the size edges.
It is a stand-alone host program built with ASan + UBSan
(`make select_plan_check`), run here as a child process."""

import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "matrixone_amd", "csrc")


def test_select_plan_check_passes_under_sanitizers():
    subprocess.run(["make", "-s", "select_plan_check"], cwd=CSRC, check=True)
    r = subprocess.run([os.path.join(CSRC, "select_plan_check")],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("select_plan_check OK"), r.stdout
