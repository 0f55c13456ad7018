"""CPU check of the scan planner (matrixone_amd/csrc/moann_scan_plan.h).

The job geometry and the kernel-variant decision of the IVF search host path
are pure integer code; scan_plan_check.cpp asserts their invariants at the
tile / group / chunk edges. It is a stand-alone host program built with
ASan + UBSan (`make scan_plan_check`), run here as a child process."""

import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "matrixone_amd", "csrc")


def test_scan_plan_check_passes_under_sanitizers():
    subprocess.run(["make", "-s", "scan_plan_check"], cwd=CSRC, check=True)
    r = subprocess.run([os.path.join(CSRC, "scan_plan_check")],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("scan_plan_check OK"), r.stdout
