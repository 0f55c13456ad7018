#!/usr/bin/env python3
"""Index BUILD timing on one MI355X: the native k-means build
(gpu_ivf_flat_build with no centroids / assignments) against the two things
it replaces, on the same rows (bench.make_mixture, [rows] x 768, nlist 4096):

  native  fused MFMA assign-argmin kernel (the default)
  gemm    MOANN_KMEANS_ASSIGN=gemm: chunked rank GEMM + top-1, the
          composition the library could already do
  torch   bench.kmeans_torch + bench.assign_torch (rocBLAS matmul Lloyd)

All three train on the same number of rows (torch's 262144-row sample; the
native build is capped to it) for the same number of iterations. The switch
is read once per process, so every run is a child process; the parent
alternates native / gemm / torch children `--runs` times and prints one JSON
line per run plus a summary. `--recall` also reports recall@10 at nprobe 32
of the natively built index next to the torch-built one (information only).

Run on a GPU box:  python tools/build_bench.py --rows 2000000 --runs 5
Not a test; writes nothing but stdout/stderr.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def log(m):
    print(m, file=sys.stderr, flush=True)


def recall_at_k(ids, gt):
    hit = 0
    for a, b in zip(ids, gt):
        hit += len(set(a.tolist()) & set(b.tolist()))
    return hit / gt.size


def child(args):
    import numpy as np
    import torch

    import bench
    from matrixone_amd import engine

    dev = torch.device("cuda:0")
    data, queries = bench.make_mixture(args.rows, args.dim, 1, 0, dev)
    torch.cuda.synchronize()
    host = data.cpu().numpy()
    n_train = min(args.rows, 262144)  # bench.kmeans_torch's sample size
    out = {"mode": args.child, "rows": args.rows, "dim": args.dim,
           "nlist": args.nlist, "iters": args.iters, "n_train": n_train}

    def build_index(cent=None, assign=None):
        ix = engine.IvfFlatIndex(args.dim, args.nlist, metric="l2sq",
                                 capacity=args.rows)
        ix.add(host)
        if cent is not None:
            ix.set_centroids(cent)
            ix.set_assignments(assign)
        else:
            ix.set_kmeans_params(args.iters, n_train)
        t0 = time.perf_counter()
        ix.build()
        return ix, (time.perf_counter() - t0) * 1e3

    def measure_recall(ix):
        q = queries[:args.recall].numpy()
        qg = torch.from_numpy(q).to(dev)
        d2 = (data * data).sum(1)[None, :] - 2.0 * (qg @ data.T)
        gt = d2.topk(args.k, dim=1, largest=False).indices.cpu().numpy()
        ids, _ = ix.search(q, args.k, args.nprobe)
        return recall_at_k(ids, gt)

    if args.child in ("native", "gemm"):
        ix, ms = build_index()
        st = ix.kmeans_stats()
        # the final assignment of every row is 2*rows*nlist*dim FLOP
        out.update(build_ms=ms, train_ms=st["train_ms"],
                   assign_ms=st["assign_ms"], iters_run=st["iters"],
                   assign_tflops=2.0 * args.rows * args.nlist * args.dim
                   / (st["assign_ms"] * 1e-3) / 1e12)
        if args.recall:
            out["recall"] = measure_recall(ix)
        ix.close()
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cent = bench.kmeans_torch(data, args.nlist, args.iters, seed=1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assign = bench.assign_torch(data, cent)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out.update(train_ms=(t1 - t0) * 1e3, assign_ms=(t2 - t1) * 1e3,
                   iters_run=args.iters)
        if args.recall:
            ix, ms = build_index(cent.cpu().numpy(),
                                 assign.cpu().numpy().astype(np.int32))
            out["pack_ms"] = ms
            out["recall"] = measure_recall(ix)
            ix.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--recall", type=int, default=0,
                    help="queries for recall@k in the first round, 0 = skip")
    ap.add_argument("--modes", default="native,gemm,torch")
    ap.add_argument("--child", choices=["native", "gemm", "torch"])
    ap.add_argument("--timeout", type=int, default=600)
    args = ap.parse_args()
    if args.child:
        return child(args)

    results = []
    for r in range(args.runs):
        for mode in args.modes.split(","):
            env = dict(os.environ)
            env.pop("MOANN_KMEANS_ASSIGN", None)
            if mode == "gemm":
                env["MOANN_KMEANS_ASSIGN"] = "gemm"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode,
                   "--rows", str(args.rows), "--dim", str(args.dim),
                   "--nlist", str(args.nlist), "--iters", str(args.iters),
                   "--k", str(args.k), "--nprobe", str(args.nprobe),
                   "--recall", str(args.recall if r == 0 else 0)]
            p = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True,
                               text=True, timeout=args.timeout)
            if p.returncode != 0:
                # a failed GPU child ends the whole measurement
                log(p.stderr[-4000:])
                sys.exit(f"build_bench: {mode} child exited {p.returncode}")
            line = p.stdout.strip().splitlines()[-1]
            res = json.loads(line)
            res["round"] = r
            results.append(res)
            print(json.dumps(res), flush=True)
    summary = {}
    for mode in args.modes.split(","):
        rs = [x for x in results if x["mode"] == mode]
        summary[mode] = {
            key: {"sorted": sorted(round(x[key], 1) for x in rs),
                  "median": round(statistics.median(x[key] for x in rs), 1)}
            for key in ("train_ms", "assign_ms")}
        rec = [x["recall"] for x in rs if "recall" in x]
        if rec:
            summary[mode]["recall"] = rec[0]
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
