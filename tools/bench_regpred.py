#!/usr/bin/env python3
"""Times the held-out scoring and many-series passes of the regression family (include/regpred.h) on one GPU.

    python tools/bench_regpred.py [--small] [--out profiles/regpred_bench.json]

Matrix rows (1e7 f32 rows, D = 16 and D = 128): ``linearregression.calc_pred_logpdf`` against ``calc_pred_dist`` plus a
torch evaluation of the Student-t on its two device arrays (what a user had before; that code path is unchanged).
Window rows (1e5 series of 200 f32 values, p = 16), for scoring and for fitting: one call with ``lengths=``, the same values
as ONE concatenated series (a different model - the floor: the same bytes without a row map), and a Python loop over the
FIRST 1000 SERIES ONLY; ``loop_extrapolated_s`` scales that figure to all series and is an extrapolation, not a measurement.
Every figure is the median of five host-clock timings of a call that ends synchronised, after one warm-up call; the
candidates of a shape alternate inside one process.  Prints one JSON line per shape.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOOP_SERIES = 1000


def timed(fns, runs=5):
    """Medians of ``runs`` timings of each callable, alternating them (one warm-up each)."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(runs):
        for fn, ts in zip(fns, out):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
    return [statistics.median(ts) for ts in out]


def matrix_rows(D, n, dev):
    from bayesml_amd import linearregression as lr
    gen = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(n, D, device=dev, generator=gen, dtype=torch.float32)
    y = x[:, 0] + torch.randn(n, device=dev, generator=gen, dtype=torch.float32)
    m = lr.LearnModel(D, device=dev).update_posterior(x[:100000], y[:100000])

    def two_arrays():
        m.calc_pred_dist(x)
        pm, pl = m._p                                   # still on the device: nothing is fetched
        nu = 2.0 * m.hn_alpha
        c0 = math.lgamma((nu + 1) / 2) - math.lgamma(nu / 2) - 0.5 * math.log(math.pi * nu)
        return c0 + 0.5 * torch.log(pl) - 0.5 * (nu + 1) * torch.log1p(pl * (y.double() - pm) ** 2 / nu)

    fused = lambda: m.calc_pred_logpdf(x, y)            # noqa: E731
    err = float((fused() - two_arrays()).abs().max())
    t_fused, t_two = timed([fused, two_arrays])
    return dict(shape=f"linearregression D = {D}, {n} f32 rows", fused_s=t_fused, pred_dist_plus_torch_s=t_two,
                max_abs_difference=err, input_bytes_per_s_fused=n * (D + 1) * 4 / t_fused)


def window_rows(p, S, length, dev):
    from bayesml_amd import autoregressive as ar
    gen = torch.Generator(device=dev).manual_seed(p)
    x = 0.3 + torch.randn(S * length, device=dev, generator=gen, dtype=torch.float32)
    lens = [length] * S
    m = ar.LearnModel(p, device=dev).update_posterior(x[:100000])
    f = ar.LearnModel(p, device=dev)
    t_score, t_score_floor = timed([lambda: m.calc_pred_logpdf(x, lengths=lens), lambda: m.calc_pred_logpdf(x)])
    t_fit, t_fit_floor = timed([lambda: f.reset_hn_params().update_posterior(x, lengths=lens),
                                lambda: f.reset_hn_params().update_posterior(x)])
    k = min(S, LOOP_SERIES)
    t_score_loop, t_fit_loop = timed([lambda: [m.calc_pred_logpdf(x[s * length:(s + 1) * length]) for s in range(k)],
                                      lambda: [f.update_posterior(x[s * length:(s + 1) * length]) for s in range(k)]], runs=3)
    return dict(shape=f"autoregressive p = {p}, {S} series of {length} f32 values", score_s=t_score,
                score_one_series_floor_s=t_score_floor, score_loop_first_series_s=t_score_loop,
                score_loop_extrapolated_s=t_score_loop * S / k, fit_s=t_fit, fit_one_series_floor_s=t_fit_floor,
                fit_loop_first_series_s=t_fit_loop, fit_loop_extrapolated_s=t_fit_loop * S / k, loop_series=k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a hundredth of the rows (a quick check of the tool itself)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    k = 100 if args.small else 1
    results = []
    for make in (lambda: matrix_rows(16, 10 ** 7 // k, dev), lambda: matrix_rows(128, 10 ** 7 // k, dev),
                 lambda: window_rows(16, 10 ** 5 // k, 200, dev)):
        results.append(make())
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
