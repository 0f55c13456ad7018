"""Child process of tests/test_refine_mfma_gpu.py::test_ab_against_dot_kernel:
runs the named refine cases, each on a fresh index, and saves what the
searches returned. The parent sets or clears MOANN_BYTE_MFMA in this
process's environment; the library reads it once per process.

usage: python refine_mfma_child.py OUT.npz CASE [CASE ...]"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import refine_cases as rc          # noqa: E402
import refine_mfma_cases as mc     # noqa: E402


def main(out, names):
    from matrixone_amd import engine
    res = {}
    for name in names:
        c = mc.lookup(name)
        cp = rc.corpus(c.kind, c.d)
        ix = engine.IvfFlatIndex(c.d, rc.NLIST, metric=c.metric,
                                 capacity=cp.vecs.shape[0])
        try:
            ix.add(cp.vecs, ids=cp.ids)
            ix.set_centroids(cp.cents)
            ix.set_assignments(cp.assign.astype(np.int32))
            ix.build()
            ix.enable_refine(c.depth)
            ids, dists = ix.search(rc.queries(c), c.k, c.probe)
        finally:
            ix.close()
        res[name + ":ids"] = np.asarray(ids)
        res[name + ":dists"] = np.asarray(dists)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
