#!/usr/bin/env python3
"""Times the Student-t mixture log-density beside the dense E-step it shares its quadratic forms with, on one MI355X:

    python tools/bench_stmix.py [--k 64] [--d 128] [--n 10000000] [--reps 10] [--warmup 2]

prints one JSON line per row dtype (f64, f32): milliseconds, median of --reps after --warmup, of
  estep_ms   the dense E-step's main kernel (estep_lds_f64) at the same K, D, N and dtype: the kernel span ``estep_main`` of
             gmmvb_profile_spans, pruning off (it writes the [K][N] ln rho array);
  logpdf_ms  stmix_logpdf alone (hipEvent timing on the stream), the image already packed;
  call_ms    StudentMixturePass.run as the models call it: pivot, c_k, stmix_pack and stmix_logpdf (hipEvent timing);
and ratio = logpdf_ms / estep_ms.  The parameters are a random well-conditioned mixture, the rows are drawn around its
means, ln p is checked finite."""
import argparse
import json
import os
import sys

import numpy as np
import torch

os.environ["GMMVB_ESTEP_PRUNE"] = "0"            # the comparison is the dense kernel
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _engine, _stmix          # noqa: E402
from bayesml_amd._regression import _code        # noqa: E402


def events(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def case(K, D, n, dtype, args, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    f64 = dict(dtype=torch.float64, device=dev)
    mu = 4.0 * torch.randn(K, D, generator=g, **f64)
    u = torch.tril(torch.randn(K, D, D, generator=g, **f64), -1) * (0.3 / D ** 0.5) + torch.eye(D, **f64) * (
        1.0 + torch.rand(K, D, generator=g, **f64))[:, :, None]
    nu = 1.0 + 8.0 * torch.rand(K, generator=g, **f64)
    pi = torch.full((K,), 1.0 / K, **f64)
    which = torch.randint(0, K, (n,), generator=g, device=dev)
    x = torch.randn(n, D, generator=g, dtype=dtype, device=dev)
    x += mu[which].to(dtype)
    del which
    row = dict(K=K, D=D, n=n, x=str(dtype).split(".")[-1])

    eng = _engine.DataPass(K, D, dtype, n, dev)
    eng.set_pivot(x[:4096].to(torch.float64).mean(dim=0))
    eng.set_params(torch.zeros(K, **f64), mu, u)
    eng.profile(True)
    spans = []
    for r in range(args.warmup + args.reps):
        eng.estep(x)
        torch.cuda.synchronize()
        if r >= args.warmup:
            spans.append(eng.kernel_spans()["estep_main"][0])
    row["estep_ms"] = round(float(np.median(spans)), 4)
    row["estep_kernel"] = eng.launch_info.split(";")[0][:80]
    eng.close()
    del eng
    torch.cuda.empty_cache()

    sm = _stmix.StudentMixturePass(K, D, dev)
    lnp, z = sm.run(x, pi, mu, nu, u, True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lnp).all()) and int(z.min()) >= 0 and int(z.max()) < K
    last, st = sm.last, _stmix.stream_ptr(dev)

    def kernel():
        rc = sm.lib.stmix_logpdf(K, D, _code(x.dtype), x.data_ptr(), x.stride(0), n, last["pivot"].data_ptr(), sm.img.data_ptr(),
                                 last["c"].data_ptr(), last["nu"].data_ptr(), lnp.data_ptr(), z.data_ptr(), st)
        assert rc == 0, sm.lib.stmix_last_error()
    row["logpdf_ms"] = round(events(kernel, args.reps, args.warmup), 4)
    row["call_ms"] = round(events(lambda: sm.run(x, pi, mu, nu, u, True), args.reps, args.warmup), 4)
    row["ratio"] = round(row["logpdf_ms"] / row["estep_ms"], 3)
    row["mean_lnp"] = round(float(lnp.mean()), 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for dtype in (torch.float64, torch.float32):
        case(args.k, args.d, args.n, dtype, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
