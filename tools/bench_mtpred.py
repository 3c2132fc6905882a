#!/usr/bin/env python3
"""Times ``metatree.LearnModel.calc_pred_logpdf`` on one MI355X:

    python tools/bench_mtpred.py [--reps 5] [--warmup 1] [--prefix 2000]

prints one JSON line per measurement: milliseconds (median of --reps after --warmup, a host clock around the whole call
ending in a synchronise; rows and results stay on the device) at (family, trees, depth, n) = (normal, 100, 5, 1e6),
(categorical of degree 16, 100, 5, 1e6), (linear regression of degree 15, 100, 5, 1e6) and (the same, 1024, 3, 1e5), on
forests of full binary trees over random continuous features, learnt from a sample of 20 000 rows with 'given_MT'.

Beside each: ``mtree_predict`` on the same adopted rows with its result LEFT ON THE DEVICE, in MEAN mode as the cost of the
walk alone (the classifier has no MEAN read-out: its PROBA mode, 16 values per row, is labelled as such), and
``calc_pred_dist(x).calc_pred_density(y)`` (the host fold, unchanged since before this pass) on the first --prefix rows,
with its extrapolation to n labelled as one.

MTPRED_SHARE is a compile-time constant.  Where variant libraries ``bayesml_amd/csrc/libgmmvb_share<k>.so`` exist (mtpred.hip
compiled with -DMTPRED_SHARE=<k> and linked with the other objects), each linear-regression shape is also timed in a child
process per library (BAYESML_AMD_LIB), the shipped library among them as share 16, two rounds in alternating order.
"""
import argparse
import ctypes
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _mtree, categorical, linearregression, metatree, normal     # noqa: E402
from bayesml_amd._native import stream_ptr     # noqa: E402


def timed(fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 4)


def tree(depth, dims, sub, rng, d=0, ranges=None):
    ranges = np.tile([-1.0, 1.0], (dims, 1)) if ranges is None else ranges
    if d == depth:
        return metatree._Node(d, sub_model=sub(), leaf=True)
    k = int(rng.integers(dims))
    lo, hi = ranges[k]
    kids = []
    for part in ((lo, 0.5 * (lo + hi)), (0.5 * (lo + hi), hi)):
        sub_ranges = ranges.copy()
        sub_ranges[k] = part
        kids.append(tree(depth, dims, sub, rng, d + 1, sub_ranges))
    return metatree._Node(d, k=k, sub_model=sub(), children=kids, thresholds=np.array([lo, 0.5 * (lo + hi), hi]))


def predict_on_device(m, xd, mode):
    """One ``mtree_predict`` launch on adopted rows; the result stays on the device."""
    eng = m._eng()
    n = int(xd.shape[0])
    out = torch.empty((n, eng.degree) if mode == _mtree.PRED_PROBA else (n,), dtype=torch.float64, device=eng.device)
    rc = eng.lib.mtree_predict(ctypes.byref(eng.struct), eng.family, eng.degree, mode, _mtree.F64, xd.data_ptr(), _mtree.U8, None, n,
                               eng.post.data_ptr(), eng.g.data_ptr(), eng.prob.data_ptr(), eng._values.data_ptr(), out.data_ptr(),
                               stream_ptr(eng.device))
    assert rc == 0, rc
    return out


SHAPES = [("normal", normal, {}, 4, 100, 5, 10 ** 6), ("categorical", categorical, {"c_degree": 16}, 4, 100, 5, 10 ** 6),
          ("linearregression", linearregression, {"c_degree": 15}, 15, 100, 5, 10 ** 6),
          ("linearregression", linearregression, {"c_degree": 15}, 15, 1024, 3, 10 ** 5)]


def emit(**row):
    print(json.dumps(row), flush=True)


def case(idx, args, dev, share=None):
    name, module, consts, dims, B, depth, n = SHAPES[idx]
    rng = np.random.default_rng(B + depth)
    sub = lambda: module.LearnModel(**consts)                                  # noqa: E731
    m = metatree.LearnModel(dims, 0, c_max_depth=depth, SubModel=module, sub_constants=consts, device=dev,
                            c_ranges=np.tile([-1.0, 1.0], (dims, 1)), h0_metatree_list=[tree(depth, dims, sub, rng) for _ in range(B)])
    gen = torch.Generator(device=dev).manual_seed(B)
    x = torch.rand(n, dims, device=dev, generator=gen, dtype=torch.float64) * 2 - 1
    y = (torch.randint(0, 16, (n,), device=dev, generator=gen) if name == "categorical"
         else x[:, 0] * 2 + torch.randn(n, device=dev, generator=gen, dtype=torch.float64))
    m.update_posterior(x[:20000], None, y[:20000], alg_type="given_MT")
    base = dict(family=name, trees=B, depth=depth, n=n)
    ms = timed(lambda: m.calc_pred_logpdf(x, None, y), args.reps, args.warmup)
    if share is not None:                     # a child process on a variant library: this one figure
        emit(what="calc_pred_logpdf", ms=ms, share=share, **base)
        return
    emit(what="calc_pred_logpdf", ms=ms, **base)
    emit(what="calc_pred_logpdf_total", ms=timed(lambda: m.calc_pred_logpdf(x, None, y, total=True), args.reps, args.warmup), **base)
    mode, label = ((_mtree.PRED_PROBA, "mtree_predict_proba_on_device") if name == "categorical"
                   else (_mtree.PRED_MEAN, "mtree_predict_mean_on_device"))
    emit(what=label, ms=timed(lambda: predict_on_device(m, x, mode), args.reps, args.warmup), **base)
    p = min(args.prefix, n)
    xh, yh = x[:p].cpu().numpy(), y[:p].cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.calc_pred_dist(xh, None).calc_pred_density(yh)
    ms = 1e3 * (time.perf_counter() - t0)
    emit(what="calc_pred_density_host_fold", rows=p, ms=round(ms, 1), extrapolated_ms_for_n=round(ms * n / p, 1), **base)
    del m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prefix", type=int, default=2000)
    ap.add_argument("--child", type=int, nargs=2, metavar=("SHAPE", "SHARE"), help="internal: one shape on the loaded library")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.child:
        return case(args.child[0], args, dev, share=args.child[1])
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesml_amd", "csrc")
    libs = {int(re.search(r"share(\d+)", f).group(1)): f for f in glob.glob(os.path.join(csrc, "libgmmvb_share*.so"))}
    if libs:
        libs[16] = os.path.join(csrc, "libgmmvb.so")
    for idx in range(len(SHAPES)):
        case(idx, args, dev)
        if SHAPES[idx][0] == "linearregression":
            for order in (sorted(libs), sorted(libs, reverse=True)):
                for k in order:
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup),
                                    "--child", str(idx), str(k)], env=dict(os.environ, BAYESML_AMD_LIB=libs[k]), check=True, timeout=300)


if __name__ == "__main__":
    main()
