#!/usr/bin/env python3
"""Golden fixtures for metatree's MTMCMC / REMTMCMC, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_metatree_mcmc.py

writes tests/golden/metatree_mcmc_<case>.npz, one per case of tests/metatree_mcmc_oracle.py: CASES.  A fixture holds the inputs,
the seed, per step the proposal's L, both truncated posteriors and the accept flag (per chain), the g_max trace (MTMCMC), the
exchange list (REMTMCMC), and the final merged list as capacity tables (feat, thr, h_g, the sub-models' posterior vectors)
with prob_vec.

The reference consumes one PCG64 stream, so a rounding-level difference in any comparison would fork the chain.  For every
case the generator therefore looks for the first seed for which EVERY comparison of the chain (keep / flip, accept, exchange,
the 2-means best against second-best cost at every node) has a relative margin of at least 1e-9, measured by the restatement
running the identical chain, and stores the smallest margin; the restatement must agree with the reference on every decision
for the seed to count.  ``ref_vs_oracle_<table>`` is the reference's deviation from the restatement, relative per array (L and
the truncated posteriors absolutely relative to |L|); the tests allow 4 x that + 64 eps.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import bernoulli, linearregression, metatree, normal          # noqa: E402
import metatree_lr_oracle as lro      # noqa: E402
import metatree_mcmc_oracle as mc     # noqa: E402
import metatree_oracle as orc         # noqa: E402

SUBS = dict(bernoulli=bernoulli, normal=normal, linearregression=linearregression)


class Traced(metatree.LearnModel):
    """The reference with the root-level values of every step recorded."""

    def start_trace(self):
        self.t_l, self.t_tp, self.t_accept = [], [], []

    def _generate_truncated_and_update(self, last, new, flag, *sample):
        v = super()._generate_truncated_and_update(last, new, flag, *sample)
        if new.depth == 0 and last is not None:
            self.t_l.append(float(v))
        return v

    def _generate_truncated_and_update_lr(self, last, new, flag, *sample):
        v = super()._generate_truncated_and_update_lr(last, new, flag, *sample)
        if new.depth == 0 and last is not None:
            self.t_l.append(float(v))
        return v

    def _calc_truncated_posterior_lean(self, node):
        v = super()._calc_truncated_posterior_lean(node)
        if node.depth == 0:
            self.t_tp.append(float(v))
        return v

    def _mh_step_truncated(self, *sample):
        before = self._num_accepted
        super()._mh_step_truncated(*sample)
        self.t_accept.append([self._num_accepted > before])

    def _remh_step_truncated_memory_efficient(self, *sample):
        top = len(self._tmp_metatree_lists[-1])
        super()._remh_step_truncated_memory_efficient(*sample)
        flags = [self._tmp_metatree_count_lists[i][-1] == 1 for i in range(self._num_chains - 1)]
        self.t_accept.append(flags + [len(self._tmp_metatree_lists[-1]) > top])


def tables_of(cfg, case, root):
    """A reference tree as capacity tables."""
    T = mc.new_tables(cfg, 1)
    stack = [(root, 0)]
    while stack:
        node, h = stack.pop()
        # (an empty child at the maximal depth keeps h0_g in the reference; the tables hold 0 at that depth, as _flatten does)
        T["g"][h] = 0.0 if node.depth == cfg.max_depth else node.h_g
        sub = node.sub_model
        if case["sub"] == "linearregression":
            T["post"][h] = lro.pack(sub.hn_mu_vec, sub.hn_lambda_mat, sub.hn_alpha, sub.hn_beta, sub._n)
        else:
            T["post"][h] = orc.post_of(cfg.fam, sub)
        if node.leaf:
            continue
        T["feat"][h] = node.k
        if node.k < cfg.dc:
            T["thr"][h, :len(node.thresholds)] = node.thresholds
        stack.extend((child, cfg.C * h + 1 + i) for i, child in enumerate(node.children))
    return T


def run_reference(case, seed):
    inp = mc.case_inputs(case)
    sub_constants = {"c_degree": case["dc"]} if case["sub"] == "linearregression" else {}
    m = Traced(case["dc"], case["dk"], c_max_depth=case["depth"], c_num_children_vec=case["C"], SubModel=SUBS[case["sub"]],
               sub_constants=sub_constants)
    m.start_trace()
    xk = inp["xk"] if case["dk"] else np.zeros((case["n"], 0), dtype=int)
    with contextlib.redirect_stdout(io.StringIO()):
        m.update_posterior(inp["xc"], xk, inp["y"], alg_type=case["alg"], threshold_type=case["threshold"], seed=seed,
                           **case["kw"])
    B = case["kw"].get("num_chains", 1)
    steps = len(m.t_accept)
    tp = np.array(m.t_tp).reshape(steps, B, 2)
    out = dict(l_new=np.array(m.t_l).reshape(steps, B), tp_new=tp[:, :, 0], tp_last=tp[:, :, 1],
               accept=np.array(m.t_accept, dtype=bool).reshape(steps, B), prob=np.array(m.hn_metatree_prob_vec))
    out["g_max"] = np.array(m._g_list) if case["alg"] == "MTMCMC" else np.zeros(0)
    out["exchange"] = np.array(m._exchange_list if case["alg"] == "REMTMCMC" else [], dtype=np.int64)
    cfg = mc.case_config(case)
    out.update({"list_" + k: v for k, v in mc.stack(cfg, [tables_of(cfg, case, r) for r in m.hn_metatree_list]).items()})
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if a.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d = np.where(a == b, 0.0, d)
    return float(np.max(d) / max(np.max(np.abs(b[np.isfinite(b)]), initial=0.0), 1e-300))


def agrees(case, ref, tr, trees, prob):
    """Every decision and structure of the restatement equals the reference's."""
    B = case["kw"].get("num_chains", 1)
    steps = len(ref["accept"])
    cfg = mc.case_config(case)
    st = mc.stack(cfg, trees)
    return (np.array_equal(np.array(tr["accept"], dtype=bool).reshape(steps, B), ref["accept"])
            and list(tr.get("exchange", [])) == list(ref["exchange"]) and st["feat"].shape == ref["list_feat"].shape
            and np.array_equal(st["feat"], ref["list_feat"]) and np.array_equal(st["thr"], ref["list_thr"]))


def main():
    for case in mc.CASES:
        for seed in range(100):
            ref = run_reference(case, seed)
            tr, trees, prob = mc.run_case(case, mc.Stream(seed))
            margin = min(tr["margins"])
            if margin >= 1e-9 and agrees(case, ref, tr, trees, prob):
                break
            print(case["name"], "seed", seed, "replaced: margin", margin)
        else:
            raise SystemExit(f"{case['name']}: no seed with a margin of 1e-9")
        B, steps = case["kw"].get("num_chains", 1), len(ref["accept"])
        st = mc.stack(mc.case_config(case), trees)
        scale = np.abs(ref["l_new"]).max()
        devs = dict(L=float(np.abs(np.array(tr["l_new"]).reshape(steps, B) - ref["l_new"]).max() / scale),
                    tp=max(rel(np.array(tr["tp_new"]).reshape(steps, B), ref["tp_new"]),
                           rel(np.array(tr["tp_last"]).reshape(steps, B), ref["tp_last"])),
                    g=rel(st["g"], ref["list_g"]), post=rel(st["post"], ref["list_post"]), prob=rel(prob, ref["prob"]),
                    g_max=rel(tr.get("g_max", []), ref["g_max"]))
        out = dict(ref, seed=np.int64(seed), margin=np.float64(margin), **mc.case_inputs(case))
        out["xk"] = out["xk"].astype(np.uint8)
        for k, v in devs.items():
            out["ref_vs_oracle_" + k] = np.float64(v)
        np.savez_compressed(os.path.join(HERE, f"metatree_mcmc_{case['name']}.npz"), **out)
        print(case["name"], "seed", seed, "steps", steps, "accepted", int(ref["accept"].sum()), "trees", len(ref["prob"]),
              "margin %.2e" % margin, devs)


if __name__ == "__main__":
    main()
