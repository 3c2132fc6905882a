"""Times ``hiddenmarkovnormal.LearnModel.calc_pred_logpdf`` on S sequences of T rows ("Predictive log-density of
many sequences"): (a) one call with ``lengths=``, (b) a Python loop of single-sequence calls over ``--loop`` of the sequences,
scaled to S and labelled as extrapolated, (c) the same rows as ONE sequence.  Host clock around calls that end in a device
synchronise; one warm-up, then ``--repeats`` timed runs each; prints one JSON line per K.

    python tools/hmmbatch_measure.py --states 32 64 --degree 16 --sequences 100000 --rows 200
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model(K, D, seed=0):
    """A model whose posterior is set by hand: well separated means, sticky transitions."""
    from bayesml_amd import hiddenmarkovnormal as hm
    rng = np.random.default_rng(seed)
    m = hm.LearnModel(K, D, seed=0, verbose=False)
    m.set_hn_params(hn_eta_vec=rng.uniform(1.0, 5.0, K), hn_zeta_vecs=rng.uniform(0.5, 5.0, (K, K)) + 6.0 * K * np.eye(K),
                    hn_m_vecs=3.0 * rng.standard_normal((K, D)), hn_kappas=rng.uniform(1.0, 9.0, K),
                    hn_nus=D + rng.uniform(0.0, 20.0, K), hn_w_mats=np.tile(np.eye(D), (K, 1, 1)))
    return m


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return dict(min_s=min(out), median_s=float(np.median(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--degree", type=int, default=16)
    ap.add_argument("--sequences", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--loop", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 35)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hmmbatch_measure needs an MI355X: a CPU run says nothing about it")
    dev = torch.device("cuda", 0)
    S, T, D = args.sequences, args.rows, args.degree
    for K in args.states:
        m = model(K, D)
        gen = torch.Generator(device=dev).manual_seed(K)
        means = torch.as_tensor(m.hn_m_vecs, device=dev)
        x = means[torch.randint(0, K, (S * T,), device=dev, generator=gen)]
        x += torch.randn(S * T, D, dtype=torch.float64, device=dev, generator=gen)
        lengths = np.full(S, T)
        kw = dict(start="initial", chunk_bytes=args.chunk_bytes)
        loop = min(args.loop, S)
        batch = timed(lambda: m.calc_pred_logpdf(x, lengths=lengths, totals=True, **kw), args.repeats)
        single = timed(lambda: m.calc_pred_logpdf(x, **kw), args.repeats)
        looped = timed(lambda: [m.calc_pred_logpdf(x[n * T:(n + 1) * T], **kw) for n in range(loop)], 1)
        a = m.calc_pred_logpdf(x[:loop * T], lengths=lengths[:loop], **kw)
        b = torch.cat([m.calc_pred_logpdf(x[n * T:(n + 1) * T], **kw) for n in range(loop)])
        print(json.dumps(dict(K=K, D=D, sequences=S, rows_each=T, dtype="f64", engine=m._hmmbatch_pass.launch_info,
                              a_batch_call=batch, c_one_sequence=single,
                              b_loop_extrapolated=dict(measured_sequences=loop, measured_s=looped["min_s"],
                                                       extrapolated_s=looped["min_s"] * S / loop),
                              max_abs_diff_batch_vs_loop=float((a - b).abs().max()))), flush=True)


if __name__ == "__main__":
    main()
