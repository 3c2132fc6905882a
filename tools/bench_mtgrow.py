#!/usr/bin/env python3
"""Time per Metropolis-Hastings step of metatree's growth engine (include/mtgrow.h) on one GPU:

    python tools/bench_mtgrow.py

n = 1e5 rows of 8 float64 features, depth 4, normal sub-model, 1 and 8 tempered chains: a whole step (growth, route, reduce,
sweep, accept and the read-back), growth alone, and route + reduce + sweep alone on the same tables - what one 'given_MT'
update of that forest costs, the floor of the scoring half.  Wall clock over 30 steps after 3 warm-up steps."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np          # noqa: E402
import torch                # noqa: E402

from bayesml_amd import _mtgrow, metatree, normal          # noqa: E402

n, F, depth = 100_000, 8, 4
rng = np.random.default_rng(0)
xc = rng.uniform(-1, 1, (n, F))
y = np.where(xc[:, 1] < 0, -1.0, 2.0) + np.where(xc[:, 3] < 0, 0.0, 1.0) + 0.3 * rng.standard_normal(n)
for B in (1, 8):
    m = metatree.LearnModel(F, 0, c_max_depth=depth, SubModel=normal, device="cuda:0")
    gr = m._grower("REMTMCMC", B, "1d_kmeans", xc, None, y)
    gr.start(_mtgrow.node_table(1, 0, B, gr.cap))
    beta = (np.arange(B) + 1) / B
    for t in range(1, 4):
        gr.step(_mtgrow.node_table(1, t, B, gr.cap), _mtgrow.aux_table(1, t, B), beta, 0.9)
    torch.cuda.synchronize()
    steps = 30
    t0 = time.perf_counter()
    for t in range(4, 4 + steps):
        gr.step(_mtgrow.node_table(1, t, B, gr.cap), _mtgrow.aux_table(1, t, B), beta, 0.9)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    # the scoring half alone on the same tables: route + reduce + sweep
    t0 = time.perf_counter()
    for _ in range(steps):
        gr.score()
    torch.cuda.synchronize()
    ds = (time.perf_counter() - t0) / steps
    # growth alone
    t0 = time.perf_counter()
    for t in range(4, 4 + steps):
        gr.grow(_mtgrow.node_table(1, t, B, gr.cap), False, 0.9)
    torch.cuda.synchronize()
    dg = (time.perf_counter() - t0) / steps
    print(f"chains {B}: step {dt * 1e3:.2f} ms, of which growth {dg * 1e3:.2f} ms, route+reduce+sweep {ds * 1e3:.2f} ms", flush=True)
    gr.close()
