#!/usr/bin/env python3
"""Exact-search timing on one MI355X: the resident brute-force index
(engine.BruteForceIndex) in its two modes against the one-shot entry it
replaces for repeated searches, on the same rows and queries:

  fused    resident rows, bf_fused_topk_kernel (MFMA distance + top-k)
  gemm     resident rows, rank GEMM into a distance tile + launch_topk
  oneshot  engine.brute_force_search: uploads the rows, packs a one-list IVF
           index, scans it and destroys it — timed whole, because that is
           what a caller pays per search today

`--storage f16` builds the resident index over an f16 row store (the fused
kernel on the f16 MFMA, gemm over a widened slice); the default f32 prints
what it always printed.

Shapes (rows x dim, nq, k): the batch shape 1M x 768 / 1024 / 10, the CDC
tail shape 10 000 x 768 / 1024 / 10, and the small batches nq 1 and nq 16 at
1M x 768. Per shape one warm-up search per mode, then `--runs` rounds that
alternate fused / gemm / oneshot; wall time per search and, for the resident
modes, the library's scan_ms / select_ms. One JSON line per run and a
summary of medians on stdout; `--out` also appends them to a .jsonl file.

Run on a GPU box:  python tools/bf_bench.py --out profiles/r05_bf_bench.jsonl
Not a test.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

SHAPES = {
    # name: (rows, dim, nq, k)
    "batch_1Mx768_nq1024": (1_000_000, 768, 1024, 10),
    "tail_10kx768_nq1024": (10_000, 768, 1024, 10),
    "small_1Mx768_nq1": (1_000_000, 768, 1, 10),
    "small_1Mx768_nq16": (1_000_000, 768, 16, 10),
}


def log(m):
    print(m, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--modes", default="fused,gemm,oneshot")
    ap.add_argument("--k", type=int, default=0, help="override every shape's k")
    ap.add_argument("--shape", action="append", default=[],
                    help="extra shape NAME=ROWS,DIM,NQ,K; replaces --shapes")
    ap.add_argument("--storage", default="f32", choices=["f32", "f16"],
                    help="row store of the resident index (oneshot stays f32)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.shape:
        extra = {}
        for spec in args.shape:
            name, _, vals = spec.partition("=")
            extra[name] = tuple(int(v) for v in vals.split(","))
        SHAPES.update(extra)
        args.shapes = ",".join(extra)

    import numpy as np
    import torch

    from matrixone_amd import engine

    assert torch.cuda.is_available(), "bf_bench needs a GPU"
    dev = torch.device("cuda:0")
    modes = args.modes.split(",")
    sink = open(args.out, "a") if args.out else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    data_cache = {}

    def rows_of(n, dim):
        if (n, dim) not in data_cache:
            data_cache.clear()  # one big host array at a time
            g = torch.Generator(device=dev).manual_seed(7)
            x = torch.randn(n, dim, generator=g, device=dev)
            data_cache[(n, dim)] = x.cpu().numpy()
            del x
            torch.cuda.empty_cache()
        return data_cache[(n, dim)]

    summary = {}
    for name in args.shapes.split(","):
        n, dim, nq, k = SHAPES[name]
        k = args.k or k
        X = rows_of(n, dim)
        Q = np.random.default_rng(3).standard_normal((nq, dim)).astype(
            np.float32)
        ix = engine.BruteForceIndex(dim, metric="l2sq", capacity=n,
                                    storage=args.storage)
        t0 = time.perf_counter()
        ix.add(X)
        add_ms = (time.perf_counter() - t0) * 1e3
        log(f"{name}: resident add of {n} rows took {add_ms:.0f} ms")

        def run(mode):
            if mode == "oneshot":
                t0 = time.perf_counter()
                ids, d = engine.brute_force_search(X, Q, k, metric="l2sq")
                return (time.perf_counter() - t0) * 1e3, None, ids, d
            ix.set_params(mode, 0)
            before = ix.perf()
            t0 = time.perf_counter()
            ids, d = ix.search(Q, k)
            wall = (time.perf_counter() - t0) * 1e3
            after = ix.perf()
            return wall, {f: after[f] - before[f]
                          for f in ("scan_ms", "select_ms", "other_ms")}, ids, d

        first = {}
        for mode in modes:  # warm-up: workspaces, code objects
            _, _, ids, d = run(mode)
            first[mode] = (ids, d)
        # information only: the three agree on the neighbours
        base = first[modes[0]][0]
        agree = {m: float((first[m][0] == base).mean()) for m in modes}

        results = []
        for r in range(args.runs):
            for mode in modes:
                wall, perf, _, _ = run(mode)
                res = {"shape": name, "rows": n, "dim": dim, "nq": nq, "k": k,
                       "mode": mode, "round": r, "wall_ms": round(wall, 3)}
                if args.storage != "f32":  # f32 lines stay as they were
                    res["storage"] = args.storage
                if perf:
                    res.update({f: round(v, 3) for f, v in perf.items()})
                results.append(res)
                emit(res)
        ix.close()
        summary[name] = {"add_ms": round(add_ms, 1), "id_agreement": agree}
        if args.storage != "f32":
            summary[name]["storage"] = args.storage
        for mode in modes:
            rs = [x for x in results if x["mode"] == mode]
            summary[name][mode] = {
                key: {"sorted": sorted(x[key] for x in rs),
                      "median": round(statistics.median(x[key] for x in rs), 3)}
                for key in ("wall_ms", "scan_ms", "select_ms") if key in rs[0]}
    emit({"summary": summary})
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
