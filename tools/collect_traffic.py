#!/usr/bin/env python3
"""Collect per-launch HBM traffic (FETCH_SIZE) for the bench's dominant
scan kernel and key it into profiles/r02_traffic.json, which bench.py emits
as `roofline.traffic` (with provenance) when the run configuration matches.

Collection per MI355X_MICROARCH.md: --pmc in its own pass (never combined
with trace domains); FETCH_SIZE is reported in KiB units per dispatch and
under-reports wide coalesced streaming reads by 2x on gfx950 — the x2
correction is applied here and stated in the provenance.

Run on a machine with the GPU (a plain bench run launches the scan kernel
often enough; `--full` is not needed):
  rocprofv3 --pmc FETCH_SIZE -d pmc_out -o traffic \
      -- python bench.py --steps 3 --warmup 1 ...
  python tools/collect_traffic.py pmc_out/*/traffic_counter_collection.csv \
      --key "10000000x768-nlist4096-nprobe32-batch1024-refine-f32" \
      --kernel scan_i8_dot --out profiles/r02_traffic.json
"""
import argparse
import csv
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv_path")
    ap.add_argument("--key", required=True)
    ap.add_argument("--kernel", default="scan_i8_dot",
                    help="substring of the dominant kernel's name")
    ap.add_argument("--min-kib", type=float, default=1e5,
                    help="ignore small launches (centroid-rank scans reuse "
                         "the same kernel at ~13 MB)")
    ap.add_argument("--out", default="profiles/r02_traffic.json")
    args = ap.parse_args()

    vals = []
    with open(args.csv_path) as f:
        for row in csv.DictReader(f):
            if args.kernel not in row["Kernel_Name"]:
                continue
            if row["Counter_Name"] != "FETCH_SIZE":
                continue
            v = float(row["Counter_Value"])
            if v < args.min_kib:
                continue
            vals.append(v)
    if not vals:
        print(f"no {args.kernel} dispatches above threshold", file=sys.stderr)
        sys.exit(1)
    mean_kib = sum(vals) / len(vals)
    bytes_per_launch = mean_kib * 1024 * 2  # x2 gfx950 correction
    db = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            db = json.load(f)
    db[args.key] = {
        "bytes_per_launch": round(bytes_per_launch),
        "launches": len(vals),
        "mean_fetch_kib_raw": round(mean_kib, 1),
        "provenance": (f"rocprofv3 --pmc FETCH_SIZE, {len(vals)} "
                       f"'{args.kernel}' dispatches, mean raw "
                       f"{mean_kib/1024/1024:.2f} GiB x2 gfx950 correction; "
                       f"csv committed under profiles/"),
    }
    with open(args.out, "w") as f:
        json.dump(db, f, indent=1)
    print(json.dumps(db[args.key]))


if __name__ == "__main__":
    main()
