#!/usr/bin/env python3
"""Golden fixtures for metatree with SubModel=linearregression, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_metatree_lr.py

writes tests/golden/metatree_lr_<case>.npz (one per case of tests/metatree_lr_oracle.py: CASES), metatree_lr_gen.npz
(GenModel under a seed) and metatree_lr_errors.json.  A fixture holds the inputs, the forest as flat tables, every node's
post vector, h_g, lml and lcm after both stages, prob_vec and the read-outs, the oracle's exact state after both stages
(``exact<stage>_*``) with the yardstick ``e_plain<stage>`` = [Lambda, beta, mu, cond_2] of tests/metatree_lr_oracle.py, and
``ref_vs_batch_*`` as
tests/golden/make_golden_metatree.py defines them: the largest deviation of the reference's recursion from the oracle's exact
batch form over the two stages (h_g in log-odds, ln prob_vec absolutely, lml relative per array), and every float read-out
against the oracle's read-out on the oracle's exact state, relative per array.

The generator asserts at every visited node that cond_2(Lambda) <= 1e3 and S_beta / beta <= 10: beyond that beta's
cancellation shows through ln beta in lml and the reference itself is no stable yardstick.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import linearregression, metatree          # noqa: E402
import metatree_lr_oracle as lro         # noqa: E402
import metatree_oracle as orc         # noqa: E402


def gen_fixture():
    """gen_params / gen_sample of GenModel under a seed: structure, thresholds, leaf parameters and the sample."""
    out = {}
    for name, kw in (("even", {}), ("random", dict(threshold_type="random"))):
        m = metatree.GenModel(2, 1, c_max_depth=3, c_num_children_vec=np.array([2, 3, 2]), SubModel=linearregression,
                              sub_constants={"c_degree": 2}, h_g=0.75, seed=7)
        m.gen_params(**kw)
        for k, v in orc.flatten_gen(m.root).items():
            out[f"{name}_{k}"] = v
        out[f"{name}_xc"], out[f"{name}_xk"], out[f"{name}_y"] = m.gen_sample(40)
    return out


def main():
    for case in lro.CASES:
        inp = lro.case_inputs(case)
        out = lro.drive(metatree, linearregression, case, inp)
        D, dc = case["D"], case["consts"]["c_dim_continuous"]
        flat = {k: out[k] for k in orc.STRUCT}
        h0 = lro.default_h0(D)
        if "init_g" not in out:          # MTRF: the state before the update, as _copy_tree_from_sklearn_tree leaves it
            out["init_g"] = np.where(flat["feat"] < 0, 0.0, 0.5)
            probe = metatree.LearnModel(SubModel=linearregression, sub_constants={"c_degree": D}, **case["consts"])
            out["init_prob"] = probe._MTRF(inp["xc1"], inp["xk1"], inp["y1"], n_estimators=8, random_state=0)[1]
        st = lro.initial_state(flat, D, h0, out["init_g"], out["init_prob"])
        ref_vs_batch = dict(g=0.0, lml=0.0, prob=0.0)
        worst = dict(cond=0.0, s_beta_over_beta=0.0)
        for stage, tag in (("after1", "1"), ("after2", "2")):
            xk = inp["xk" + tag] if case["consts"]["c_dim_categorical"] else None
            before = st
            st, counts, info = lro.batch_update(flat, st, D, h0, dc, inp["xc" + tag], xk, inp["y" + tag])
            # the exact state and the yardstick e_plain travel with the fixture, so that no test repeats the mpmath pass
            plain = lro.plain_update(flat, before, D, h0, dc, inp["xc" + tag], xk, inp["y" + tag])
            e_plain = lro.post_errs(plain["post"], st["post"], D, info, counts > 0)
            for k in orc.STATE:
                out[f"exact{tag}_{k}"] = st[k]
            out[f"exact{tag}_counts"], out[f"exact{tag}_s_beta"], out[f"exact{tag}_lam_scale"] = counts, info["s_beta"], info["lam_scale"]
            out[f"e_plain{tag}"] = np.array([e_plain[k] for k in ("lam", "beta", "mu", "cond")])
            for v in np.flatnonzero(counts > 0):
                _, lam, _, beta, _ = lro.unpack(st["post"][v], D)
                worst["cond"] = max(worst["cond"], float(np.linalg.cond(lam)))
                worst["s_beta_over_beta"] = max(worst["s_beta_over_beta"], info["s_beta"][v] / beta)
            assert worst["cond"] <= 1e3 and worst["s_beta_over_beta"] <= 10, (case["name"], worst)
            errs = lro.state_errs({k: out[f"{stage}_{k}"] for k in orc.STATE}, st)
            ref_vs_batch = {k: max(ref_vs_batch[k], errs[k]) for k in errs}
            assert np.array_equal(np.isnan(st["lml"]), np.isnan(out[f"{stage}_lml"])), (case["name"], stage)
        for k, v in lro.oracle_readouts(flat, st, case, inp).items():
            ref_vs_batch[k] = orc.rel_err(out[k], v)
        for k, v in ref_vs_batch.items():
            out["ref_vs_batch_" + k] = np.float64(v)
        for k, v in inp.items():
            out[k] = v.astype(np.uint8) if k.startswith("xk") else v
        np.savez_compressed(os.path.join(HERE, f"metatree_lr_{case['name']}.npz"), **out)
        print(case["name"], "trees", len(flat["tree_off"]) - 1, "nodes", len(flat["feat"]), worst, "ref_vs_batch", ref_vs_batch)
    np.savez_compressed(os.path.join(HERE, "metatree_lr_gen.npz"), **gen_fixture())
    errors = {name: orc.outcome(fn) for name, fn in lro.error_cases(metatree, linearregression).items()}
    with open(os.path.join(HERE, "metatree_lr_errors.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
    print(errors)


if __name__ == "__main__":
    main()
