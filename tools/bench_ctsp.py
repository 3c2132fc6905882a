#!/usr/bin/env python3
"""Times the three phases of the sparse context-tree update on one MI355X:

    python tools/bench_ctsp.py [--n 10000000] [--reps 10] [--warmup 2]

prints one JSON line per case: milliseconds (median of --reps after --warmup, hipEvent timing on the stream) of ctsp_count
(with the zeroing of the scratch that it starts with), ctsp_levelup and ctsp_sweep, each timed alone on a tree that the
untimed phases before it have prepared, at (c_k, c_d_max) = (4, 8) - which tools/bench_ctree.py times on the dense engine -
(4, 16) and (256, 4) for an independent uniform uint8 sample, and at (4, 8) and (4, 16) for an all-equal sample (one hot
key per level).  Rows are dense in c_k, so a case whose tables would exceed the engine's memory budget is retried at a
tenth of the length; the line says which n ran."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _ctsp                    # noqa: E402
from bayesml_amd._engine import EngineLimitError  # noqa: E402


def timed(prep, fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def case(k, D, n, sample, args, dev):
    eng = _ctsp.SparseCtreePass(k, D, dev)
    while True:
        try:
            eng._reserve(n)
            break
        except EngineLimitError:
            n //= 10
    x = (torch.randint(0, k, (n,), dtype=torch.uint8, device=dev) if sample == "uniform"
         else torch.ones(n, dtype=torch.uint8, device=dev))
    hb = np.ones(k) / 2
    row = dict(c_k=k, c_d_max=D, n=n, sample=sample, slots=eng.off[-1],
               table_gib=round(eng.off[-1] * eng.slot_bytes / 2 ** 30, 2))

    def counted():
        eng.clear()
        eng.count(x)

    def raised():
        counted()
        eng.levelup(x)
    row["count_ms"] = round(timed(eng.clear, lambda: eng.count(x), args.reps, args.warmup), 4)
    row["levelup_ms"] = round(timed(counted, lambda: eng.levelup(x), args.reps, args.warmup), 4)
    row["sweep_ms"] = round(timed(raised, lambda: eng.sweep(x, 0.5, hb), args.reps, args.warmup), 4)
    row["nodes"] = int((eng.exists != 0).sum())
    assert [int(v) for v in eng._status[:3].cpu()] == [n, 0, 0]
    print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for k, D, sample in ((4, 8, "uniform"), (4, 8, "all_equal"), (4, 16, "uniform"), (4, 16, "all_equal"),
                         (256, 4, "uniform")):
        case(k, D, args.n, sample, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
