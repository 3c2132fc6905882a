#!/usr/bin/env python3
"""Times ``contexttree.LearnModel.calc_pred_logpdf`` on one MI355X:

    python tools/bench_ctpred.py [--reps 5] [--warmup 1] [--loop 2000]

prints one JSON line per measurement: milliseconds (median of --reps after --warmup, a host clock around the whole call
ending in a synchronise; samples and results stay on the device) of

* ``calc_pred_logpdf`` alone and with ``assign=True`` at (c_k, c_d_max, n) = (2, 10, 1e6), (4, 6, 1e6), (256, 2, 1e5) on
  dense tables and (4, 16, 1e6), (256, 4, 1e5) on sparse tables, each after an ``update_posterior`` of a sample of the same
  length, for an independent uniform held-out sample; the row-sum prepass (``ctpred_rowsum_*``) alone; on sparse tables
  both up-walks (the LDS stack and the probing one), also for the training sample itself as held-out sample, whose paths
  never leave the tree;
* for comparison ``pred_and_update_sequence(loss=None, code_length=True)`` at the dense shapes (it learns, so every
  repetition starts from a copy of the model, copied outside the clock), and the per-position ``calc_pred_dist`` loop over
  the first --loop positions, with its extrapolation to n labelled as one;
* a batch of 1e4 sequences of 100 symbols at (4, 6) with ``totals=True``.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _ctpred, contexttree     # noqa: E402


def timed(fn, reps, warmup, prep=None):
    ms = []
    for r in range(warmup + reps):
        arg = prep() if prep is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg) if prep is not None else fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 4)


def emit(**row):
    print(json.dumps(row), flush=True)


def case(k, D, n, tables, args, dev):
    gen = torch.Generator(device=dev).manual_seed(k * 1000 + D)
    x = torch.randint(0, k, (n,), dtype=torch.uint8, device=dev, generator=gen)
    y = torch.randint(0, k, (n,), dtype=torch.uint8, device=dev, generator=gen)
    m = contexttree.LearnModel(k, D, tables=tables, device=dev).update_posterior(x)
    base = dict(c_k=k, c_d_max=D, n=n, tables=tables)
    m.calc_pred_logpdf(y[:1000])                 # (creates the pass)
    pp, eng = m._pred_pass, m._eng()
    hb = torch.as_tensor(m.hn_beta_vec, device=dev)
    emit(what="rowsum_prepass", slots=int(m._store.pred_tables(eng)["off"][-1]),
         ms=timed(lambda: pp.row_sums(m._store.pred_tables(eng), True, hb), args.reps, args.warmup), **base)
    walks = (("stack", _ctpred.UP_STACK), ("probe", _ctpred.UP_PROBE)) if tables == "sparse" else ((None, pp.upwalk),)
    helds = (("uniform", y), ("training_sample", x)) if tables == "sparse" else (("uniform", y),)
    for held, sample in helds:
        for walk, code in walks:
            pp.upwalk = code
            extra = dict(heldout=held, **({"upwalk": walk} if walk else {}))
            emit(what="calc_pred_logpdf", ms=timed(lambda: m.calc_pred_logpdf(sample), args.reps, args.warmup), **extra, **base)
            emit(what="calc_pred_logpdf_assign", ms=timed(lambda: m.calc_pred_logpdf(sample, assign=True), args.reps, args.warmup),
                 **extra, **base)
    pp.upwalk = _ctpred.PredPass.upwalk
    if tables == "dense":
        emit(what="pred_and_update_sequence_code_length",
             ms=timed(lambda c: c.pred_and_update_sequence(y, loss=None, code_length=True), args.reps, args.warmup,
                      prep=lambda: copy.deepcopy(m)), **base)
    loop, yh = copy.deepcopy(m), y[:args.loop].cpu().numpy().astype(np.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(len(yh)):
        loop.calc_pred_dist(yh[:i + 1])
    torch.cuda.synchronize()
    per = 1e3 * (time.perf_counter() - t0) / len(yh)
    emit(what="calc_pred_dist_loop", positions=len(yh), ms_per_position=round(per, 4),
         extrapolated_ms_for_n=round(per * n, 1), **base)
    del m, loop
    torch.cuda.empty_cache()


def batch(args, dev):
    k, D, S, L = 4, 6, 10_000, 100
    gen = torch.Generator(device=dev).manual_seed(7)
    x = torch.randint(0, k, (S * L,), dtype=torch.uint8, device=dev, generator=gen)
    y = torch.randint(0, k, (S * L,), dtype=torch.uint8, device=dev, generator=gen)
    m = contexttree.LearnModel(k, D, device=dev).update_posterior(x)
    lengths = np.full(S, L, dtype=np.int64)
    emit(what="batch_totals", c_k=k, c_d_max=D, sequences=S, symbols_each=L, tables="dense",
         ms=timed(lambda: m.calc_pred_logpdf(y, lengths=lengths, totals=True), args.reps, args.warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop", type=int, default=2000)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for k, D, n, tables in ((2, 10, 10 ** 6, "dense"), (4, 6, 10 ** 6, "dense"), (256, 2, 10 ** 5, "dense"),
                            (4, 16, 10 ** 6, "sparse"), (256, 4, 10 ** 5, "sparse")):
        case(k, D, n, tables, args, dev)
    batch(args, dev)


if __name__ == "__main__":
    main()
