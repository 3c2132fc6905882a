#!/usr/bin/env python3
"""Times ``pred_and_update_sequence`` of multivariate_normal on one GPU against the per-row loop it replaces and against
the regression sequence pass at the same size.

    python tools/bench_mvnseq.py [--out profiles/mvnseq_bench.json]

D = 16, 64, 128, 256 with n = 1e6 f32 rows on the device.  Per shape: the median of five timed calls after one warm-up, for
``loss=None, code_length=True`` (no [n, D] array) and for ``loss="squared"`` (with the means); each call includes the
final update_posterior pass and its host inverse, and ends synchronised.  The per-row loop (``pred_and_update`` row by row)
runs over the FIRST 2000 ROWS ONLY; ``loop_extrapolated_s`` scales that figure to n rows and is an extrapolation, not a
measurement.  ``regseq_nats_s`` is linearregression's ``pred_and_update_sequence(loss=None, code_length=True)`` on the
same matrix with a random target: the same block work with one read of x fewer, so the ratio shows what the centring costs.
Prints one JSON line per shape.
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


def shape(D, n, dev):
    from bayesml_amd import linearregression as lr, multivariate_normal as mvn
    rng = np.random.default_rng(0)
    x = 0.5 + rng.standard_normal((n, D), dtype=np.float32)
    xd = torch.from_numpy(x).to(dev)
    yd = torch.from_numpy(rng.standard_normal(n, dtype=np.float32)).to(dev)
    m, r = mvn.LearnModel(D, device=dev), lr.LearnModel(D, device=dev)

    def seq(**kw):
        m.reset_hn_params()
        m.pred_and_update_sequence(xd, **kw)

    def regseq():
        r.reset_hn_params()
        r.pred_and_update_sequence(xd, yd, loss=None, code_length=True)

    def loop():
        lm = mvn.LearnModel(D, device=dev)
        x64 = x[:LOOP_ROWS].astype(np.float64)
        for i in range(min(LOOP_ROWS, n)):
            lm.pred_and_update(x64[i])
    return seq, regseq, loop, m, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a hundredth of the rows (a quick check of the tool itself)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 10 ** 6 // (100 if args.small else 1)
    results = []
    for D in (16, 64, 128, 256):
        seq, regseq, loop, m, r = shape(D, n, dev)
        res = dict(D=D, rows=n, seq_nats_s=timed(lambda: seq(loss=None, code_length=True)),
                   seq_squared_s=timed(lambda: seq(loss="squared")), launches=m._seq_engine.launch_info,
                   regseq_nats_s=timed(regseq), regseq_launches=r._seq_engine.launch_info)
        res["rows_per_s_nats"] = n / res["seq_nats_s"]
        res["rows_per_s_squared"] = n / res["seq_squared_s"]
        res["seq_over_regseq"] = res["seq_nats_s"] / res["regseq_nats_s"]
        loop()                                   # warm-up
        torch.cuda.synchronize()
        t = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        res["loop_first_2000_rows_s"] = time.perf_counter() - t
        res["loop_extrapolated_s"] = res["loop_first_2000_rows_s"] * n / min(LOOP_ROWS, n)
        res["speedup_vs_extrapolated_loop"] = res["loop_extrapolated_s"] / res["seq_squared_s"]
        results.append(res)
        print(json.dumps(res), flush=True)
        del seq, regseq, loop, m, r
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
