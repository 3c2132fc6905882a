#!/usr/bin/env python3
"""Times ``contexttree.LearnModel.update_posterior(x, lengths=...)`` on one MI355X:

    python tools/bench_ctfit.py [--reps 5] [--warmup 1] [--loop 1000]

prints one JSON line per measurement: milliseconds (median of --reps after --warmup, a host clock around the whole call
ending in a synchronise; the symbols stay on the device as uint8; every repetition starts from a fresh model made
outside the clock) at (c_k, c_d_max) = (4, 8) and (2, 10) for 1e5 sequences of 200 symbols of

* the many-sequence call, and its parts: ``ctfit_count`` with the host read, the two sorts, ``ctfit_rank``, ``ctfit_sweep``;
* the single-sequence ``update_posterior`` of the concatenation of the same symbols (another model: the floor);
* a Python loop of single-sequence updates over the first --loop sequences, with its extrapolation to all of them
  labelled as one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesml_amd import _ctfit, contexttree     # noqa: E402
from bayesml_amd._ctree import _CODES           # noqa: E402
from bayesml_amd._native import stream_ptr      # noqa: E402


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


def parts(m, x, seq_off, args, base):
    """The stages of ``_ctfit.FitPass.update`` one by one on a model that has been updated once (so the pass exists)."""
    fp, eng, dev = m._fit_pass, m._eng(), x.device
    lib, k, D = fp.lib, fp.k, fp.D
    hoff = _ctfit.head_offsets(seq_off, D)
    H, S, n = int(hoff[-1]), len(seq_off) - 1, int(x.shape[0])
    seq, hof = torch.as_tensor(seq_off, device=dev), torch.as_tensor(hoff, device=dev)
    hb = torch.as_tensor(m.hn_beta_vec, device=dev)
    keys = torch.empty(2, H, dtype=torch.int64, device=dev)
    head = torch.empty(int(lib.ctfit_head_len(H)), dtype=torch.int64, device=dev)
    sample = (_CODES[x.dtype], x.data_ptr(), n, seq.data_ptr(), hof.data_ptr(), S, H, k, D)
    st = stream_ptr(dev)

    def count():
        assert lib.ctfit_count(*sample, eng._out.data_ptr(), keys.data_ptr(), fp._work.data_ptr(), st) == 0
        return eng._out[:2].cpu()

    count()
    ordered = torch.stack([torch.sort(keys[0]).values, torch.sort(keys[1]).values])
    emit(what="ctfit_count_and_read", heads=H, ms=timed(count, args.reps, args.warmup), **base)
    emit(what="two_sorts", heads=H, ms=timed(lambda: (torch.sort(keys[0]), torch.sort(keys[1])), args.reps, args.warmup), **base)
    emit(what="ctfit_rank", ms=timed(lambda: lib.ctfit_rank(*sample, ordered.data_ptr(), eng.beta.data_ptr(), eng.exists.data_ptr(),
                                                            hb.data_ptr(), head.data_ptr(), fp._work.data_ptr(), st),
                                     args.reps, args.warmup), **base)
    emit(what="ctfit_sweep", ms=timed(lambda: lib.ctfit_sweep(k, D, eng._out.data_ptr() + 16, eng.beta.data_ptr(), eng.g.data_ptr(),
                                                              eng.exists.data_ptr(), float(m.hn_g), hb.data_ptr(),
                                                              fp._work.data_ptr(), st), args.reps, args.warmup), **base)


def case(k, D, S, L, args, dev):
    gen = torch.Generator(device=dev).manual_seed(k * 1000 + D)
    x = torch.randint(0, k, (S * L,), dtype=torch.uint8, device=dev, generator=gen)
    lengths = np.full(S, L, dtype=np.int64)
    base = dict(c_k=k, c_d_max=D, sequences=S, symbols_each=L)

    def fresh():
        m = contexttree.LearnModel(k, D, device=dev)
        m._eng()
        return m

    emit(what="update_posterior_lengths", ms=timed(lambda m: m.update_posterior(x, lengths=lengths), args.reps, args.warmup, prep=fresh), **base)
    emit(what="update_posterior_concatenated_floor", ms=timed(lambda m: m.update_posterior(x), args.reps, args.warmup, prep=fresh), **base)
    m = fresh().update_posterior(x, lengths=lengths)
    parts(m, x, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), args, base)
    loop, rows = fresh(), x[:args.loop * L].view(args.loop, L)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.loop):
        loop.update_posterior(rows[s])
    torch.cuda.synchronize()
    per = 1e3 * (time.perf_counter() - t0) / args.loop
    emit(what="single_sequence_loop", sequences_timed=args.loop, ms_per_sequence=round(per, 4),
         extrapolated_ms_for_all=round(per * S, 1), **base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop", type=int, default=1000)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for k, D in ((4, 8), (2, 10)):
        case(k, D, 100_000, 200, args, dev)


if __name__ == "__main__":
    main()
