#!/usr/bin/env python3
"""The scalar conjugate data passes (include/expfam.h) on one MI355X, each over a device tensor of --bytes bytes.

Not the headline metric (bench.py is); this is the measurement behind profiles/expfam_bench.md.  Per family and dtype, in
one process and alternating between them: the pass itself (``ExpfamPass.stats``: two kernels, no read-back), the model's
``update_posterior`` (the pass, the read-back of the block and the host closed form), a device-to-device copy of the same
tensor (the streaming ceiling: it reads and writes every byte) and ``torch.sum`` of it.  Times are device-event times,
median and range over --reps after --warmup.  GB/s is the tensor's bytes over the median; ``vs_copy_read`` is the pass's
rate over the copy's READ rate (bytes / copy time).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def summary(ms, nbytes):
    med = float(np.median(ms))
    return dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), gb_per_s=round(nbytes / med / 1e6, 1))


def chunks(n, fn, dtype, dev, step=1 << 26):
    """A tensor of n values made piecewise (fn(count) -> values), so that no temporary is larger than the result."""
    out = torch.empty(n, dtype=dtype, device=dev)
    for i in range(0, n, step):
        out[i:i + step] = fn(min(step, n - i)).to(dtype)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_expfam.py needs an MI355X: a timing taken elsewhere says nothing")
    from bayesml_amd import _expfam as xf
    from bayesml_amd import bernoulli, categorical, exponential, normal, poisson
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(20251018)
    eng = xf.ExpfamPass(dev)
    B = args.bytes

    def rand(c):
        return torch.rand(c, generator=g, device=dev)

    def index(degree, dtype):
        n = B // torch.empty(0, dtype=dtype).element_size()
        return chunks(n, lambda c: (rand(c) * degree).to(torch.int64).clamp_(max=degree - 1), dtype, dev)

    def onehot(degree):
        rows = B // degree
        x = torch.zeros((rows, degree), dtype=torch.uint8, device=dev)
        step = max(1, (1 << 26) // degree)
        for i in range(0, rows, step):
            c = min(step, rows - i)
            x[i:i + c].scatter_(1, (rand(c) * degree).to(torch.int64).clamp_(max=degree - 1)[:, None], 1)
        return x

    cases = [("bernoulli", "uint8", xf.BERNOULLI, 0, lambda: chunks(B, lambda c: rand(c) < 0.3, torch.uint8, dev),
              lambda: bernoulli.LearnModel(device=dev), {}),
             ("bernoulli", "int32", xf.BERNOULLI, 0, lambda: chunks(B // 4, lambda c: rand(c) < 0.3, torch.int32, dev),
              lambda: bernoulli.LearnModel(device=dev), {})]
    for degree in (2, 16, 1000):
        dt = torch.uint8 if degree <= 256 else torch.int32
        cases.append((f"categorical index c_degree={degree}", str(dt).split(".")[1], xf.COUNTS, degree,
                      lambda degree=degree, dt=dt: index(degree, dt),
                      lambda degree=degree: categorical.LearnModel(degree, device=dev), dict(onehot=False)))
        cases.append((f"categorical one-hot c_degree={degree}", "uint8", xf.ONEHOT, degree, lambda degree=degree: onehot(degree),
                      lambda degree=degree: categorical.LearnModel(degree, device=dev), {}))
    cases += [
        ("poisson", "uint8", xf.POISSON, 0, lambda: chunks(B, lambda c: torch.poisson(torch.full((c,), 4.0, device=dev), generator=g),
                                                           torch.uint8, dev), lambda: poisson.LearnModel(device=dev), {}),
        ("poisson", "int32", xf.POISSON, 0, lambda: chunks(B // 4, lambda c: torch.poisson(torch.full((c,), 4.0, device=dev), generator=g),
                                                           torch.int32, dev), lambda: poisson.LearnModel(device=dev), {}),
        ("poisson (mean 1000: lgamma off the table)", "int32", xf.POISSON, 0,
         lambda: chunks(B // 4, lambda c: torch.poisson(torch.full((c,), 1000.0, device=dev), generator=g), torch.int32, dev),
         lambda: poisson.LearnModel(device=dev), {}),
        ("exponential", "float32", xf.EXPONENTIAL, 0, lambda: chunks(B // 4, lambda c: -torch.log1p(-rand(c)) + 1e-6, torch.float32, dev),
         lambda: exponential.LearnModel(device=dev), {}),
        ("exponential", "float64", xf.EXPONENTIAL, 0, lambda: chunks(B // 8, lambda c: -torch.log1p(-rand(c)) + 1e-6, torch.float64, dev),
         lambda: exponential.LearnModel(device=dev), {}),
        ("normal", "float32", xf.NORMAL, 0, lambda: chunks(B // 4, lambda c: 3.0 + 2.0 * torch.randn(c, generator=g, device=dev),
                                                          torch.float32, dev), lambda: normal.LearnModel(device=dev), {}),
        ("normal", "float64", xf.NORMAL, 0,
         lambda: chunks(B // 8, lambda c: 1e8 + torch.randn(c, generator=g, device=dev, dtype=torch.float64), torch.float64, dev),
         lambda: normal.LearnModel(device=dev), {}),
    ]
    out = dict(bench="expfam", device=torch.cuda.get_device_name(0), bytes=B, reps=args.reps, warmup=args.warmup, cases=[])
    for name, dtype, family, degree, make, model, kw in cases:
        x = make()
        nbytes = x.numel() * x.element_size()
        dst = torch.empty_like(x)
        m = model()
        xa = eng.adopt(x, "f" if family in (xf.EXPONENTIAL, xf.NORMAL) else "i", cols=degree if family == xf.ONEHOT else None)
        assert xa.data_ptr() == x.data_ptr()
        t = timed({"pass": lambda: eng.stats(family, xa, degree), "update_posterior": lambda: m.update_posterior(x, **kw),
                   "copy": lambda: dst.copy_(x), "torch_sum": lambda: torch.sum(x)}, args.reps, args.warmup)
        res = {k: summary(v, nbytes) for k, v in t.items()}
        res.update(family=name, dtype=dtype, values=x.numel(), bytes=nbytes,
                   vs_copy_read=round(float(np.median(t["copy"]) / np.median(t["pass"])), 3))
        out["cases"].append(res)
        del x, dst, xa, m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
