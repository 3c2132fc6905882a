#!/usr/bin/env python3
"""Times the HMM sequence predictive beside the fit's own emission + forward-backward pass at the same shape, on one MI355X:

    python tools/bench_hmmpred.py [--k 32] [--d 16] [--t 10000000] [--reps 7] [--warmup 2] [--fit-itr 3] [--trace]

A sequence is drawn on the device from a GenModel (transitions that stay with 0.9, means four spreads apart), a LearnModel
is fitted for --fit-itr iterations, and one JSON line is printed: milliseconds, median of --reps after --warmup, HIP events
on the stream, one process, of
  fit_pass_ms  the yardstick: gmmvb_estep (emission) + hmmvb_forward_backward of the fitted model's engine over the rows;
  stmix_ms     stmix_logpdf over the same rows and parameters (the emission's yardstick: same quadratic forms);
  call_ms      HmmFilterPass.run over the whole sequence in one slice: c_k, stmix_pack and hmmpred_logpdf, ln p and z;
  method_ms    LearnModel.calc_pred_logpdf(x, assign=True) as a user calls it (default chunk_bytes: time slices);
diag = the call's diagnostic (chunks whose start did not stand, chunks walked again), ratio = call_ms / fit_pass_ms.
--trace runs each of the three device paths twice and nothing else, for a kernel trace taken around the tool."""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _hmmpred, _stmix, hiddenmarkovnormal as hm          # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--t", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fit-itr", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    K, D, T = args.k, args.d, args.t
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    a = np.full((K, K), 0.1 / max(1, K - 1))
    np.fill_diagonal(a, 0.9 if K > 1 else 1.0)
    gen = hm.GenModel(K, D, a_mat=a, mu_vecs=4.0 * rng.standard_normal((K, D)), seed=1)
    x, _ = gen.gen_sample(T, device=dev)
    m = hm.LearnModel(K, D, seed=0, device=dev, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.update_posterior(x, max_itr=args.fit_itr, num_init=1)
    eng, xd = m._engine, m._x_dev
    q = m._post_tensors(dev)

    def fit_pass():
        eng.set_params(q.c, q.m, q.u)
        eng.estep(xd)
        eng.forward_backward(q.pi_tilde, q.a_tilde)

    m.calc_pred_dist()
    t = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev)          # noqa: E731
    scale = m.hn_kappas * m.p_nus / (m.hn_kappas + 1)
    u = torch.sqrt(t(scale))[:, None, None] * _stmix.precision_factor(t(m.hn_w_mats_inv))
    am, mu, nu = t(m.p_a_mat), t(m.p_mu_vecs), t(m.p_nus)
    w0 = t(m.hn_eta_vec / m.hn_eta_vec.sum())
    fp = _hmmpred.HmmFilterPass(K, D, dev)
    sm = _stmix.StudentMixturePass(K, D, dev)
    lnp, z, end, diag = fp.run(xd, am, w0, mu, nu, u, True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lnp).all()) and int(z.min()) >= 0 and int(z.max()) < K
    row = dict(K=K, D=D, T=T, x=str(xd.dtype).split(".")[-1], plan=_hmmpred.default_plan(T), diag=diag.tolist(),
               sum_lnp=float(lnp.sum()), scratch_gb=round(8 * _hmmpred.scratch_len(K, D, T) / 2 ** 30, 2))
    del lnp, z
    if args.trace:
        for fn in (fit_pass, lambda: sm.run(xd, w0, mu, nu, u, False), lambda: fp.run(xd, am, w0, mu, nu, u, True)):
            fn()
            fn()
            torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        return
    row["fit_pass_ms"] = round(events(fit_pass, args.reps, args.warmup), 3)
    row["stmix_ms"] = round(events(lambda: sm.run(xd, w0, mu, nu, u, False), args.reps, args.warmup), 3)
    row["call_ms"] = round(events(lambda: fp.run(xd, am, w0, mu, nu, u, True), args.reps, args.warmup), 3)
    row["call_no_z_ms"] = round(events(lambda: fp.run(xd, am, w0, mu, nu, u, False), args.reps, args.warmup), 3)
    row["method_ms"] = round(events(lambda: m.calc_pred_logpdf(xd, start="initial", assign=True), args.reps, args.warmup), 3)
    row["ratio"] = round(row["call_ms"] / row["fit_pass_ms"], 3)
    row["steps_per_s"] = round(T / row["call_ms"] * 1e3, 1)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
