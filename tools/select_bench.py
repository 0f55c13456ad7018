#!/usr/bin/env python3
"""Micro-benchmark of the ragged per-query selection kernels alone
(moann_select_topk): the radix select against the threshold filter at the
flagship's shape, 1024 rows of about 78 000 candidates, k = 64.

Rows are ragged (a seeded +-5 % around --count) and hold what the refine
first pass writes: integer-valued f32 distances of one query, which share
their high bits (--dist bytes), or plain Gaussians (--dist gauss). Each mode
is launched --reps times after one warm-up launch; the time is the device
time of the one kernel (HIP events inside moann_select_topk), the rate is the
candidate bytes over it. One JSON line per mode:

  {"mode", "ms_median", "ms_min", "ms_all", "gbs", "bytes", "fallbacks",
   "fallback_rate", "rows", "k", "same_as_radix"}

Needs the GPU."""

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_rows(nq, count, dist, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    counts = rng.integers(int(count * 0.95), int(count * 1.05) + 1, nq)
    qoffs = np.zeros(nq + 1, dtype=np.int64)
    qoffs[1:] = np.cumsum(counts)
    d = rng.standard_normal(int(qoffs[-1]), dtype=np.float32)
    if dist == "bytes":
        # squared byte distances over 768 dims: integers near 2.5e6 with a
        # spread of a few per cent, per-query offset
        base = np.repeat(rng.uniform(2.0e6, 3.0e6, nq).astype(np.float32),
                         counts)
        d = np.rint(base + np.float32(1.2e5) * d).astype(np.float32)
    return d, qoffs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--count", type=int, default=78000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dist", choices=["bytes", "gauss"], default="bytes")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()

    from matrixone_amd import engine
    d, qoffs = make_rows(args.rows, args.count, args.dist, args.seed)
    nbytes = int(d.size) * 4
    ref = None
    for mode in ("radix", "filter"):
        times, fb, out = [], 0, None
        for rep in range(args.reps + 1):
            s, dd, fb, ms = engine.select_topk(d, qoffs, args.k, mode)
            if rep:
                times.append(ms)
            out = (s, dd)
        if ref is None:
            ref = out
        med = statistics.median(times)
        print(json.dumps({
            "mode": mode, "ms_median": round(med, 4),
            "ms_min": round(min(times), 4),
            "ms_all": [round(t, 4) for t in times],
            "gbs": round(nbytes / 1e9 / (med / 1e3), 1), "bytes": nbytes,
            "fallbacks": fb, "fallback_rate": round(fb / args.rows, 5),
            "rows": args.rows, "k": args.k, "dist": args.dist,
            "same_as_radix": bool(
                np.array_equal(out[0], ref[0]) and
                np.array_equal(out[1].view(np.uint32),
                               ref[1].view(np.uint32)))}), flush=True)


if __name__ == "__main__":
    main()
