#!/usr/bin/env python3
"""bench.py, unchanged and with its own arguments, plus one more output line:
IvfFlatIndex.select_stats() of the benchmark's index, printed just before the
index closes — how many queries of the run the threshold-filter selection
finished and how many it handed back to the radix select
(`{"select_stats": {"filtered": ..., "fallback": ...}}`). Needs the GPU."""

import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from matrixone_amd import engine
    close = engine.IvfFlatIndex.close

    def close_with_stats(self):
        print(json.dumps({"select_stats": self.select_stats()}), flush=True)
        close(self)

    engine.IvfFlatIndex.close = close_with_stats
    sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
