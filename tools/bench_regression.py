#!/usr/bin/env python3
"""The regression data passes (include/regvb.h) on one MI355X: statistics, predictive read-out, lag-window loader.

Not the headline metric (bench.py is); this is the measurement behind DESIGN.md's regression subsection
(profiles/regression_bench.md).  Per shape (D, N), f32 rows:

  stats     regvb_stats, against the only route the engine had to the same sums before: DataPass(1, D + 1),
            load_responsibilities(ones) once, gmmvb_mstep on a pre-concatenated [x | y] matrix - timed in the same process,
            alternating with it; also that route at D - 1 regressors (so that both sides run the same number of feature
            tiles when D is a multiple of 16), and both end to end (update_posterior vs cat + ones + mstep).
  predict   regvb_predict; for context torch f64  x @ Linv^T, square, row sum  on the same device.
  window    regvb_stats_window at T = --series, p = --degree-ar.

Times are device-event times of the whole call (its kernels and the gaps between them), median and range over --reps
after --warmup.  FLOP counts are what the kernels EXECUTE (whole 16 x 16 x 4 MFMA tiles: upper tile pairs of the Gram
matrix, the lower block triangle of the factor, feature tiles rounded up to an even count) and the share of peak is
against the f64 MFMA rate tools/peak_probe measures on this GPU (its best +0 line), not a data-sheet number.  Prints
one JSON line.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def probe_peak():
    """Best f64 MFMA rate (TFLOP/s) of tools/peak_probe's pure-MFMA lines, or None if the probe is not built."""
    exe = os.path.join(ROOT, "tools", "peak_probe")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    rates = [float(m.group(1)) for m in re.finditer(r"\+0 v_fma_f64/MFMA.*?([0-9.]+) TFLOP/s\(mfma\)", out)]
    return max(rates) if rates else None


def timed(fns, reps, warmup):
    """Device-event milliseconds of each callable in ``fns``, alternating between them; {name: [ms] * reps}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def summary(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def even_tiles(D):
    return 2 * ((D + 31) // 32)


def bench_shape(D, N, args, dev, peak):
    from bayesml_amd import linearregression as lr
    from bayesml_amd._engine import DataPass
    from bayesml_amd._normalgamma import inverse_factor
    from bayesml_amd._regression import RegressionPass
    gen = torch.Generator(device=dev).manual_seed(20251016)
    x = torch.randn(N, D, device=dev, generator=gen, dtype=torch.float32)
    theta = torch.randn(D, device=dev, generator=gen, dtype=torch.float32) / D ** 0.5
    y = x @ theta + 0.5 * torch.randn(N, device=dev, generator=gen, dtype=torch.float32)
    res = dict(D=D, N=N, dtype="float32")
    eng = RegressionPass(D, dev)

    # ---- statistics against the K = 1 M-step route
    xy = torch.cat([x, y[:, None]], dim=1).contiguous()
    ones = torch.ones((N, 1), dtype=torch.float64, device=dev)
    old = DataPass(1, D + 1, torch.float32, N, dev)
    old.set_pivot(torch.zeros(D + 1, dtype=torch.float64, device=dev))
    old.load_responsibilities(ones)
    old_m1 = DataPass(1, D, torch.float32, N, dev)          # D - 1 regressors + y
    old_m1.set_pivot(torch.zeros(D, dtype=torch.float64, device=dev))
    old_m1.load_responsibilities(ones)
    xy_m1 = xy[:, 1:].contiguous()
    model = lr.LearnModel(D, device=dev)

    def old_end_to_end():
        m = torch.cat([x, y[:, None]], dim=1)
        old.load_responsibilities(torch.ones((N, 1), dtype=torch.float64, device=dev))
        return old.mstep(m).cpu()

    t = timed({"regvb_stats": lambda: eng.stats(x, y), "mstep_k1": lambda: old.mstep(xy),
               "mstep_k1_one_column_less": lambda: old_m1.mstep(xy_m1)}, args.reps, args.warmup)
    T = even_tiles(D)
    flop = 512.0 * (T * (T + 1) // 2) * N
    ms = float(np.median(t["regvb_stats"]))
    res["stats"] = dict(regvb_stats=summary(t["regvb_stats"]), mstep_k1=summary(t["mstep_k1"]),
                        mstep_k1_one_column_less=summary(t["mstep_k1_one_column_less"]),
                        mstep_k1_kernels=[k.split(" grid=")[0] for k in old.launch_info.split(" | ") if k][:1],
                        executed_gflop=round(flop / 1e9, 2), tflops=round(flop / ms / 1e9, 2),
                        share_of_probe_peak=None if peak is None else round(flop / ms / 1e9 / peak, 3),
                        bytes_gb=round(4.0 * N * (D + 1) / 1e9, 3), tb_per_s=round(4.0 * N * (D + 1) / ms / 1e9, 3))
    # the new statistics equal the old route's (G = B, c = a column, s = B corner about a zero pivot)
    ns, _h, a, B = old.split_stats(old.mstep(xy))
    s_new = eng.stats(x, y)
    G_old = B[0][:D, :D].reshape(-1)
    res["stats"]["max_rel_diff_to_mstep_k1"] = float(((s_new[:D * D] - G_old).abs().max() / G_old.abs().max()).item())
    t = timed({"update_posterior": lambda: model.update_posterior(x, y), "cat_ones_mstep": old_end_to_end},
              max(3, args.reps // 4), 2)
    res["stats"]["end_to_end"] = {k: summary(v) for k, v in t.items()}
    old.close()
    old_m1.close()
    del xy, xy_m1, ones

    # ---- predictive read-out
    model.fit(x, y)
    linv = inverse_factor(model.hn_lambda_mat)
    linv_t = torch.from_numpy(linv).to(dev).T.contiguous()
    scale = model.hn_alpha / model.hn_beta

    def torch_route():
        z = x.to(torch.float64) @ linv_t
        return scale / (1.0 + (z * z).sum(dim=1))

    t = timed({"regvb_predict": lambda: eng.predict(x, model.hn_mu_vec, linv, scale), "torch_f64": torch_route},
              args.reps, args.warmup)
    flop = 256.0 * T * (T + 1) * N
    ms = float(np.median(t["regvb_predict"]))
    res["predict"] = dict(regvb_predict=summary(t["regvb_predict"]), torch_f64=summary(t["torch_f64"]),
                          executed_gflop=round(flop / 1e9, 2), executed="lower block triangle only (D^2 per row, not 2 D^2)",
                          tflops=round(flop / ms / 1e9, 2),
                          share_of_probe_peak=None if peak is None else round(flop / ms / 1e9 / peak, 3),
                          note="regvb_predict's time includes the upload of mu / Linv and a stream synchronise")
    pl = eng.predict(x, model.hn_mu_vec, linv, scale)[1]
    res["predict"]["max_rel_diff_to_torch"] = float(((pl - torch_route()).abs().max() / pl.abs().max()).item())
    eng.close()
    return res


def bench_window(args, dev):
    from bayesml_amd._regression import PAD_NONE, RegressionPass
    p, T = args.degree_ar, args.series
    gen = torch.Generator(device=dev).manual_seed(3)
    e = torch.randn(T + 1, device=dev, generator=gen, dtype=torch.float64)
    x = 0.3 + e[1:] + 0.6 * e[:-1]
    eng = RegressionPass(p + 1, dev)
    t = timed({"regvb_stats_window": lambda: eng.stats_window(x, PAD_NONE)}, args.reps, args.warmup)
    res = dict(p=p, T=T, dtype="float64", regvb_stats_window=summary(t["regvb_stats_window"]),
               series_mb=round(8.0 * T / 1e6, 1))
    if args.ref_rows:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import regression_oracle as orc
        xs = x[:args.ref_rows].cpu().numpy()
        t0 = time.perf_counter()
        w, yv = orc.lag_matrix(xs, p, None)
        orc.update(np.zeros(p + 1), np.eye(p + 1), 1.0, 1.0, w, yv)
        res["numpy_restatement_cpu_s"] = dict(rows=args.ref_rows, seconds=round(time.perf_counter() - t0, 3),
                                              note="vectorised NumPy restatement of the update on this host's CPU, not the "
                                                   "reference's Python loop over T")
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x10000000,64x12500000", help="comma-separated DxN")
    ap.add_argument("--series", type=int, default=10_000_000)
    ap.add_argument("--degree-ar", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regression.py needs an MI355X: a timing taken elsewhere says nothing")
    peak = probe_peak()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    out = dict(bench="regression", device=torch.cuda.get_device_name(0), probe_peak_f64_mfma_tflops=peak, reps=args.reps,
               shapes=[], window=None)
    for spec in args.shapes.split(","):
        D, N = (int(v) for v in spec.split("x"))
        out["shapes"].append(bench_shape(D, N, args, dev, peak))
    out["window"] = bench_window(args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
