#!/usr/bin/env python3
"""Times the meta-tree forest engine on one MI355X:

    python tools/bench_mtree.py [--n 1000000] [--trees 100] [--depth 8] [--reps 20] [--warmup 5]

prints one JSON line per sub-model (bernoulli, normal, linearregression; --subs picks some): milliseconds (median of --reps after --warmup, hipEvent timing on
the stream) of mtree_route, mtree_reduce, mtree_sweep and of the three together, and of mtree_predict, on --n rows of 8
continuous float32 features through --trees full binary trees of depth --depth (a random feature per node, the threshold in
the middle of the node's range).  route_gbs is the traffic the route pass cannot avoid -- the rows once and one int32 stop
node per (row, tree) -- over its time.  linearregression regresses on all 8 features: its reduction is mtree_reduce_x (the
ordering, the segmented Gram pass and the fix-up in one call; a kernel trace splits them), its row also has predict_var_ms,
and gram_gbs is the bytes the Gram pass gathers -- per (row, tree) the row's features, its y and its sorted index -- over the
whole reduction's time.

    python tools/bench_mtree.py --reference /path/to/BayesML --n 100000

times the reference's update_posterior(alg_type='given_MT') and predict on the same forest on the host CPU instead (one run
each; not part of the product)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def forest_tables(n_trees, depth, dim, rng):
    feat, child0, nchild, thr_off, dep, thr, tree_off = [], [], [], [], [], [], [0]
    for _ in range(n_trees):
        base = len(feat)
        ranges = [np.tile([-3.0, 3.0], (dim, 1))]
        for v in range(2 ** (depth + 1) - 1):
            d = int(np.log2(v + 1))
            dep.append(d)
            if d == depth:
                feat.append(-1), child0.append(0), nchild.append(0), thr_off.append(-1)
                continue
            k = int(rng.integers(dim))
            lo, hi = ranges[v][k]
            feat.append(k), child0.append(base + 2 * v + 1), nchild.append(2), thr_off.append(len(thr))
            thr.extend([lo, (lo + hi) / 2, hi])
            for side in (0, 1):
                r = ranges[v].copy()
                r[k, 1 - side] = (lo + hi) / 2
                ranges.append(r)
        tree_off.append(len(feat))
    i32 = lambda a: np.array(a, np.int32)       # noqa: E731
    return dict(tree_off=i32(tree_off), feat=i32(feat), child0=i32(child0), nchild=i32(nchild), thr_off=i32(thr_off),
                depth=i32(dep), thr=np.array(thr))


def run_reference(path, args, tabs, x, ys):
    sys.path.insert(0, path)
    os.environ.setdefault("MPLBACKEND", "Agg")
    from bayesml import bernoulli, linearregression, metatree, normal
    import metatree_oracle as orc
    for name, sub in (("bernoulli", bernoulli), ("normal", normal), ("linearregression", linearregression)):
        if name not in args.subs:
            continue
        consts = {"c_degree": 8} if sub is linearregression else {}
        m = metatree.LearnModel(8, 0, c_max_depth=args.depth, SubModel=sub, sub_constants=consts)
        g = np.where(tabs["feat"] < 0, 0.0, 0.5)
        m.set_hn_params(hn_metatree_list=orc.nodes_from_flat(metatree, tabs, g, lambda: sub.LearnModel(**consts)))
        x64 = x.astype(np.float64)
        t0 = time.perf_counter()
        m.update_posterior(x64, None, ys[name], alg_type="given_MT")
        t1 = time.perf_counter()
        m.predict(x64, None)
        t2 = time.perf_counter()
        print(json.dumps(dict(reference=name, n=args.n, trees=args.trees, depth=args.depth,
                              update_ms=round(1e3 * (t1 - t0), 1), predict_ms=round(1e3 * (t2 - t1), 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--subs", default="bernoulli,normal,linearregression")
    args = ap.parse_args()
    args.subs = args.subs.split(",")
    rng = np.random.default_rng(0)
    tabs = forest_tables(args.trees, args.depth, 8, rng)
    x = rng.uniform(-3, 3, (args.n, 8)).astype(np.float32)
    ys = dict(bernoulli=(rng.random(args.n) < 0.5 + 0.1 * np.sign(x[:, 0])).astype(np.int64),
              normal=x[:, 0].astype(np.float64) + rng.standard_normal(args.n))
    ys["linearregression"] = ys["normal"]
    if args.reference:
        return run_reference(args.reference, args, tabs, x, ys)
    import torch
    from bayesml_amd import _mtree
    from bench_ctree import timed
    dev = torch.device("cuda", 0)
    flat = _mtree.FlatForest(**tabs)
    xd = torch.from_numpy(x).to(dev)
    lr_h0 = np.concatenate([np.zeros(8), np.eye(8)[np.triu_indices(8)], [1.0, 1.0, 0.0]])
    for name, fam, h0, mode in (("bernoulli", _mtree.BERNOULLI, [0.5, 0.5], _mtree.PRED_PROBA),
                                ("normal", _mtree.NORMAL, [0.0, 1.0, 1.0, 1.0, 0.0], _mtree.PRED_MEAN),
                                ("linearregression", _mtree.LINREG, lr_h0, _mtree.PRED_MEAN)):
        if name not in args.subs:
            continue
        lr = fam == _mtree.LINREG
        eng = _mtree.MtreePass(flat, fam, 8 if lr else 0, 8, 0, [], h0, dev)
        reduce = (lambda: eng.reduce_x(stop, xd, y)) if lr else (lambda: eng.reduce(stop, y))
        start = dict(g=np.where(flat.feat < 0, 0.0, 0.5), post=np.tile(h0, (flat.n_nodes, 1)), lml=np.full(flat.n_nodes, np.nan),
                     lcm=np.zeros(flat.n_nodes), prob=np.ones(flat.n_trees) / flat.n_trees)
        eng.set_state(start)
        y = eng.adopt_y(ys[name])
        stop = eng.route(xd, None)[0]
        row = dict(sub_model=name, n=args.n, trees=args.trees, depth=args.depth, nodes=flat.n_nodes)
        row["route_ms"] = round(timed(lambda: eng.route(xd, None), args.reps, args.warmup), 4)
        row["reduce_ms"] = round(timed(reduce, args.reps, args.warmup), 4)
        row["sweep_ms"] = round(timed(lambda: eng.sweep(), args.reps, args.warmup), 4)
        eng.set_state(start)

        def update():
            nonlocal stop
            stop = eng.route(xd, None)[0]
            reduce()
            eng.sweep()
        row["update_ms"] = round(timed(update, args.reps, args.warmup), 4)
        row["predict_ms"] = round(timed(lambda: eng.predict(xd, None, mode), args.reps, args.warmup), 4)
        row["route_gbs"] = round((x.nbytes + 4 * args.n * args.trees) / row["route_ms"] / 1e6, 1)
        if lr:
            row["predict_var_ms"] = round(timed(lambda: eng.predict(xd, None, _mtree.PRED_VAR), args.reps, args.warmup), 4)
            row["gram_gbs"] = round(args.n * args.trees * (8 * 4 + 8 + 4) / row["reduce_ms"] / 1e6, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
