"""CPU check of the k-means build rules (matrixone_amd/csrc/moann_kmeans_plan.h).

The sample, init, reseed and stop rules of the native k-means build are pure
host arithmetic and part of the documented build contract;
kmeans_plan_check.cpp asserts them at their edges (n == nlist,
n_train == nlist, a fraction giving n_train < nlist, the cap, ties in reseed,
more empty centroids than distinct far rows). It is a stand-alone host program
built with ASan + UBSan (`make kmeans_plan_check`), run here as a child
process."""

import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "matrixone_amd", "csrc")


def test_kmeans_plan_check_passes_under_sanitizers():
    subprocess.run(["make", "-s", "kmeans_plan_check"], cwd=CSRC, check=True)
    r = subprocess.run([os.path.join(CSRC, "kmeans_plan_check")],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("kmeans_plan_check OK"), r.stdout
