#!/usr/bin/env python3
"""Times ``pred_and_update_sequence`` of autoregressive / linearregression on one GPU against the per-row loop it replaces.

    python tools/bench_regseq.py [--out profiles/regseq_bench.json]

Three shapes: AR(15) on 1e6 f32 values, D = 64 with n = 1e6 rows (f32), D = 256 with n = 1e5 rows (f32).  Per shape: the
median of five timed calls after one warm-up, for ``loss=None, code_length=True`` and for ``loss="squared"`` (each call
includes the final update_posterior pass and its host solve, and ends synchronised), and the per-row loop
(``pred_and_update`` row by row) over the FIRST 2000 ROWS ONLY; ``loop_extrapolated_s`` scales that figure to n rows and is
an extrapolation, not a measurement.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOOP_ROWS = 2000


def timed(fn, runs=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return statistics.median(out)


def shape_ar(p, n, dev):
    from bayesml_amd import autoregressive as ar
    rng = np.random.default_rng(0)
    x = (0.3 + rng.standard_normal(n)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    make = lambda: ar.LearnModel(p, device=dev)      # noqa: E731
    m = make()

    def seq(**kw):
        m.reset_hn_params()
        m.pred_and_update_sequence(xd, **kw)

    def loop():
        lm = make()
        x64 = x[:LOOP_ROWS + p].astype(np.float64)
        for t in range(p, LOOP_ROWS + p):
            lm.pred_and_update(x64[t - p:t + 1])
    return f"AR({p}), {n} f32 values", n - p, seq, loop, m


def shape_lr(D, n, dev):
    from bayesml_amd import linearregression as lr
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, D), dtype=np.float32)
    y = (x @ rng.standard_normal(D).astype(np.float32) + rng.standard_normal(n, dtype=np.float32))
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    make = lambda: lr.LearnModel(D, device=dev)      # noqa: E731
    m = make()

    def seq(**kw):
        m.reset_hn_params()
        m.pred_and_update_sequence(xd, yd, **kw)

    def loop():
        lm = make()
        for i in range(LOOP_ROWS):
            lm.pred_and_update(x[i], float(y[i]))
    return f"linearregression D = {D}, n = {n} f32 rows", n, seq, loop, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a hundredth of the rows (a quick check of the tool itself)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    k = 100 if args.small else 1
    results = []
    for make in (lambda: shape_ar(15, 10 ** 6 // k, dev), lambda: shape_lr(64, 10 ** 6 // k, dev),
                 lambda: shape_lr(256, 10 ** 5 // k, dev)):
        name, n, seq, loop, m = make()
        res = dict(shape=name, rows=n,
                   seq_nats_s=timed(lambda: seq(loss=None, code_length=True)),
                   seq_squared_s=timed(lambda: seq(loss="squared")), launches=m._seq_engine.launch_info)
        loop()                                   # warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        res["loop_first_2000_rows_s"] = time.perf_counter() - t
        res["loop_extrapolated_s"] = res["loop_first_2000_rows_s"] * n / LOOP_ROWS
        res["speedup_vs_extrapolated_loop"] = res["loop_extrapolated_s"] / res["seq_squared_s"]
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
