#!/usr/bin/env python3
"""Times the scalar conjugate families' prequential pass (include/expseq.h) on one MI355X:

    python tools/bench_expseq.py [--n 100000000] [--reps 5] [--warmup 2]

prints one JSON line per case: milliseconds (median of --reps after --warmup, hipEvent timing on the stream) of the pass
asked for the code lengths alone (``loss=None, code_length=True``) and for what the default loss needs (the parameter arrays;
for categorical the rows, at --rows-n positions of c_degree 64), and beside each the one-read statistics pass
``ExpfamPass.stats`` of the parent on the same array in the same process.  ``hbm_share`` is the bytes the algorithm must move
(the sample read twice, every requested array written once at 8 bytes an entry) over the time, as a share of the 8 TB/s HBM3E
peak of the MI355X.  Samples are made on the device from a seed; scratch and outputs are allocated inside the timed call,
as the models' calls do."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _expfam as xf            # noqa: E402
from bayesml_amd import _expseq as xs            # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s


def timed(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        del out
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)


def sample(family, n, dtype, dev, gen, degree=0):
    if family == "bernoulli":
        return torch.randint(0, 2, (n,), dtype=dtype, device=dev, generator=gen)
    if family == "poisson":
        return torch.poisson(torch.full((n,), 3.7, device=dev), generator=gen).to(dtype)
    if family == "categorical":
        return torch.randint(0, degree, (n,), dtype=torch.int32 if degree > 256 else dtype, device=dev, generator=gen)
    if family == "exponential":
        return torch.empty(n, dtype=dtype, device=dev).exponential_(0.5, generator=gen) + 1e-3
    return torch.randn(n, dtype=dtype, device=dev, generator=gen)


SCALAR = {"bernoulli": (xs.BERNOULLI, xf.BERNOULLI, (0.5, 0.5)), "poisson": (xs.POISSON, xf.POISSON, (1.0, 1.0)),
          "exponential": (xs.EXPONENTIAL, xf.EXPONENTIAL, (1.0, 1.0)), "normal": (xs.NORMAL, xf.NORMAL, (0.0, 1.0, 1.0, 1.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rows-n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    seq, stats = xs.SequencePass(dev), xf.ExpfamPass(dev)
    cases = [("bernoulli", torch.uint8), ("poisson", torch.uint8), ("exponential", torch.float32), ("exponential", torch.float64),
             ("normal", torch.float32), ("normal", torch.float64)]
    for name, dtype in cases:
        fam, stat_fam, start = SCALAR[name]
        x = sample(name, args.n, dtype, dev, gen)
        n, size, n_par = args.n, x.element_size(), len(xs.PARAMS[fam])
        row = dict(family=name, dtype=str(dtype).split(".")[1], n=n)
        row["nats_ms"] = round(timed(lambda: seq.run(fam, x, start, params=False, nats=True), args.reps, args.warmup), 3)
        row["nats_hbm_share"] = share(n * (2 * size + 8), row["nats_ms"])
        row["default_loss_ms"] = round(timed(lambda: seq.run(fam, x, start, params=True, nats=False), args.reps, args.warmup), 3)
        row["default_loss_hbm_share"] = share(n * (2 * size + 8 * n_par), row["default_loss_ms"])
        row["stats_ms"] = round(timed(lambda: stats.stats(stat_fam, x), args.reps, args.warmup), 3)
        row["stats_hbm_share"] = share(n * size, row["stats_ms"])
        assert int(seq.run(fam, x, start, params=False, nats=False)[2].cpu()[0]) == 0
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    for degree in (16, 4096):
        x = sample("categorical", args.n, torch.uint8, dev, gen, degree)
        alpha = np.ones(degree) / 2
        row = dict(family="categorical", c_degree=degree, dtype=str(x.dtype).split(".")[1], n=args.n)
        row["nats_ms"] = round(timed(lambda: seq.run_categorical(x, False, alpha, None, True), args.reps, args.warmup), 3)
        row["passes"] = seq.passes
        row["nats_hbm_share"] = share(args.n * (2 * x.element_size() + 8), row["nats_ms"])
        row["stats_ms"] = round(timed(lambda: stats.stats(xf.COUNTS, x, degree), args.reps, args.warmup), 3)
        row["stats_hbm_share"] = share(args.n * x.element_size(), row["stats_ms"])
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    degree, n = 64, args.rows_n
    x = sample("categorical", n, torch.uint8, dev, gen, degree)
    alpha = np.ones(degree) / 2
    row = dict(family="categorical", c_degree=degree, dtype="uint8", n=n)
    row["default_loss_ms"] = round(timed(lambda: seq.run_categorical(x, False, alpha, "rows", False), args.reps, args.warmup), 3)
    row["passes"] = seq.passes
    row["default_loss_hbm_share"] = share(n * (2 + 8 * degree), row["default_loss_ms"])
    row["argmax_ms"] = round(timed(lambda: seq.run_categorical(x, False, alpha, "argmax", False), args.reps, args.warmup), 3)
    row["stats_ms"] = round(timed(lambda: stats.stats(xf.COUNTS, x, degree), args.reps, args.warmup), 3)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
