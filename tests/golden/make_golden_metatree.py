#!/usr/bin/env python3
"""Golden fixtures for metatree, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_metatree.py

writes tests/golden/metatree_<case>.npz (one per case of tests/metatree_oracle.py: CASES), metatree_gen.npz (GenModel under
a seed) and metatree_errors.json.  A fixture holds the inputs, the forest as flat tables (so that the GPU tests replay it
with 'given_MT' and do not depend on the scikit-learn version), every node's posterior, h_g, lml and lcm after both stages,
prob_vec and the read-outs.

Per case the fixture also records ``ref_vs_batch``: the largest deviation of the reference's recursion from the oracle's exact
batch form over the two stages -- h_g in log-odds, ln prob_vec absolutely (entries above 1e-300), post and lml relative per
array; and for every float read-out (predict / predict_proba, pred_var, pred_density, feature_importances) the reference's
read-out against the oracle's read-out on the oracle's state, relative per array.  The tests read their tolerances from them.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import bernoulli, categorical, exponential, metatree, normal, poisson          # noqa: E402
import metatree_oracle as orc         # noqa: E402

SUBS = dict(bernoulli=bernoulli, categorical=categorical, poisson=poisson, exponential=exponential, normal=normal)


def gen_fixture():
    """gen_params / gen_sample of GenModel under a seed: structure, integers and floats of the reference."""
    out = {}
    for name, sub, kw in (("bern", bernoulli, {}), ("norm", normal, dict(threshold_type="random"))):
        m = metatree.GenModel(2, 1, c_max_depth=3, c_num_children_vec=np.array([2, 3, 2]), SubModel=sub, h_g=0.75, seed=7)
        m.gen_params(**kw)
        flat = orc.flatten_gen(m.root)
        xc, xk, y = m.gen_sample(40)
        for k, v in flat.items():
            out[f"{name}_{k}"] = v
        out[f"{name}_xc"], out[f"{name}_xk"], out[f"{name}_y"] = xc, xk, y
    return out


def main():
    for case in orc.CASES:
        inp = orc.case_inputs(case)
        out = orc.drive(metatree, SUBS, case, inp)
        fam = orc.FAMILY[case["sub"]]
        flat = {k: out[k] for k in orc.STRUCT}
        dc = case["consts"]["c_dim_continuous"]
        degree = case.get("sub_constants", {}).get("c_degree", 0)
        h0 = orc.post_of(fam, SUBS[case["sub"]].LearnModel(**case.get("sub_constants", {})))
        if "init_g" not in out:          # MTRF: the state before the update, as _copy_tree_from_sklearn_tree leaves it
            leaf = flat["feat"] < 0
            out["init_g"] = np.where(leaf, 0.0, 0.5)
            # prob after the merge of equal trees, before the update (the forest is deterministic under random_state)
            probe = metatree.LearnModel(SubModel=SUBS[case["sub"]], sub_constants=case.get("sub_constants", {}), **case["consts"])
            out["init_prob"] = probe._MTRF(inp["xc1"], inp["xk1"], inp["y1"], n_estimators=8, random_state=0)[1]
        st = dict(g=out["init_g"], post=np.tile(h0, (len(flat["feat"]), 1)), lml=np.full(len(flat["feat"]), np.nan),
                  lcm=np.zeros(len(flat["feat"])), prob=out["init_prob"])
        ref_vs_batch = dict(g=0.0, post=0.0, lml=0.0, prob=0.0)
        for stage, tag in (("after1", "1"), ("after2", "2")):
            st, _ = orc.batch_update(flat, st, fam, degree, h0, dc, inp["xc" + tag], inp["xk" + tag], inp["y" + tag])
            errs = orc.state_errs({k: out[f"{stage}_{k}"] for k in orc.STATE}, st)
            ref_vs_batch = {k: max(ref_vs_batch[k], errs[k]) for k in errs}
            assert np.array_equal(np.isnan(st["lml"]), np.isnan(out[f"{stage}_lml"])), (case["name"], stage)
        for k, v in ref_vs_batch.items():
            out["ref_vs_batch_" + k] = np.float64(v)
        # the float read-outs: the reference's against the oracle's on the oracle's exact state, relative per array
        for k, v in orc.oracle_readouts(flat, st, case, inp).items():
            out["ref_vs_batch_" + k] = np.float64(orc.rel_err(out[k], v))
            ref_vs_batch[k] = float(out["ref_vs_batch_" + k])
        for k, v in inp.items():
            out[k] = v.astype(np.uint8) if k.startswith("xk") else v
        np.savez_compressed(os.path.join(HERE, f"metatree_{case['name']}.npz"), **out)
        print(case["name"], "trees", len(flat["tree_off"]) - 1, "nodes", len(flat["feat"]), "ref_vs_batch", ref_vs_batch)
    np.savez_compressed(os.path.join(HERE, "metatree_gen.npz"), **gen_fixture())
    errors = {name: orc.outcome(fn) for name, fn in orc.error_cases(metatree, SUBS).items()}
    with open(os.path.join(HERE, "metatree_errors.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
    print(sum(v is not None for v in errors.values()), "of", len(errors), "boundary cases raise")


if __name__ == "__main__":
    main()
