#!/usr/bin/env python3
"""Times ctree_count and ctree_sweep on one MI355X:

    python tools/bench_ctree.py [--n 10000000] [--reps 20] [--warmup 5]

prints one JSON line per shape: milliseconds (median of --reps after --warmup, hipEvent timing on the stream) of the count
and of the sweep at (c_k, c_d_max) = (2, 10) - the LDS-histogram path - and (4, 8) - the global-integer-atomic path - for an
independent uniform sample and for an all-equal sample (one hot context: every add of a workgroup hits one bin); and at
(256, 1), the widest alphabet, whose root is one lane that walks 256 x 256 child counts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _ctree          # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for k, D in ((2, 10), (4, 8), (256, 1)):
        eng = _ctree.CtreePass(k, D, dev)
        hb = np.ones(k) / 2
        row = dict(c_k=k, c_d_max=D, n=args.n, path="lds" if k ** (D + 1) <= 4096 else "global_atomics")
        for name, x in (("uniform", torch.randint(0, k, (args.n,), dtype=torch.uint8, device=dev)),
                        ("all_equal", torch.ones(args.n, dtype=torch.uint8, device=dev))):
            row[f"count_ms_{name}"] = round(timed(lambda: eng.count(x), args.reps, args.warmup), 4)

            def sweep():
                eng.clear()
                eng.sweep(x, 0.5, hb)
            row[f"sweep_ms_{name}"] = round(timed(sweep, args.reps, args.warmup), 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
