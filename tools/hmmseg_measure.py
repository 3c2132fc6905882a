"""Times a VB iteration of ``hiddenmarkovnormal.LearnModel.update_posterior`` over S sequences of T rows (DESIGN.md, §4c
"Fit from many sequences"): with ``lengths=`` (the segment kernels) and the same S T rows as ONE sequence (the chunk-parallel
path), in the same session.  Host clock around whole calls of ``--short`` and ``--long`` iterations (tolerance 0: none
converges); the difference over the iterations between them is the iteration, free of the set-up.  One JSON line per K.

    python tools/hmmseg_measure.py --states 32 64 --degree 16 --sequences 100000 --rows 200

``--decode`` times ``estimate_latent_vars``'s engine calls on the same rows instead (``decode_ms``):

    python tools/hmmseg_measure.py --decode --states 4 16 32 64 --degree 16 --sequences 100000 --rows 200
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def iteration_ms(m, x, lengths, short, long_, repeats):
    def fit(itr):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = time.perf_counter()
            m.update_posterior(x, max_itr=itr, num_init=1, tolerance=0.0, lengths=lengths)
            torch.cuda.synchronize()
            return time.perf_counter() - t
    fit(short)                                                   # warm-up
    per = [(fit(long_) - fit(short)) / (long_ - short) * 1e3 for _ in range(repeats)]
    return dict(min_ms=min(per), median_ms=float(np.median(per)))


def decode_ms(K, D, S, T, x, means, repeats, loop_sequences):
    """The ``--decode`` leg ("Decoding many sequences"): the S sequences decoded by one ``viterbi_segments``
    call, the same S T rows decoded as ONE sequence by ``viterbi`` (the chunk-parallel pass), both after the same E-step on
    one engine with the host clock around the synchronising calls; and ``estimate_latent_vars`` looped in Python over the
    first ``loop_sequences`` sequences, extrapolated to S."""
    from bayesml_amd import hiddenmarkovnormal as hm
    m = hm.LearnModel(K, D, seed=0, verbose=False)
    m.set_hn_params(hn_m_vecs=means.cpu().numpy())
    eng, xd = m._open(x)
    eng.enable_hmm()
    eng.emission_target(False)
    q = m._post_tensors(xd.device)
    eng.set_params(q.c, q.m, q.u)
    eng.estep(xd)
    off_dev, order_dev = eng.segment_tables(T * np.arange(S + 1, dtype=np.int64))

    def clock(call):
        call()                                                   # warm-up
        per = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            per.append((time.perf_counter() - t) * 1e3)
        return dict(min_ms=min(per), median_ms=float(np.median(per)))

    seg = clock(lambda: eng.viterbi_segments(q.ln_pi_tilde, q.ln_a_tilde, off_dev, order_dev))
    one = clock(lambda: eng.viterbi(q.ln_pi_tilde, q.ln_a_tilde))
    n = min(loop_sequences, S)
    m.estimate_latent_vars(x[:T])                                # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    for s in range(n):
        m.estimate_latent_vars(x[s * T:(s + 1) * T])
    loop_s = (time.perf_counter() - t) / n * S
    return dict(K=K, D=D, sequences=S, rows_each=T, dtype="f64", segments=seg, one_sequence=one,
                python_loop_extrapolated_s=loop_s, looped=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", action="store_true", help="time the decode of the batch instead of the fit")
    ap.add_argument("--loop-sequences", type=int, default=1000)
    ap.add_argument("--states", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--degree", type=int, default=16)
    ap.add_argument("--sequences", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hmmseg_measure needs an MI355X: a CPU run says nothing about it")
    from bayesml_amd import hiddenmarkovnormal as hm
    dev = torch.device("cuda", 0)
    S, T, D = args.sequences, args.rows, args.degree
    for K in args.states:
        gen = torch.Generator(device=dev).manual_seed(K)
        means = 3.0 * torch.randn(K, D, dtype=torch.float64, device=dev, generator=gen)
        x = means[torch.randint(0, K, (S * T,), device=dev, generator=gen)]
        x += torch.randn(S * T, D, dtype=torch.float64, device=dev, generator=gen)
        if args.decode:
            print(json.dumps(decode_ms(K, D, S, T, x, means, args.repeats, args.loop_sequences)), flush=True)
            continue
        m = hm.LearnModel(K, D, seed=0, verbose=False)
        seg = iteration_ms(m, x, np.full(S, T), args.short, args.long, args.repeats)
        one = iteration_ms(m, x, None, args.short, args.long, args.repeats)
        print(json.dumps(dict(K=K, D=D, sequences=S, rows_each=T, dtype="f64", iterations=[args.short, args.long],
                              segments=seg, one_sequence=one)), flush=True)


if __name__ == "__main__":
    main()
