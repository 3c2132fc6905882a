#!/usr/bin/env python3
"""Golden fixtures for contexttree beyond the dense-table limit, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_contexttree_sparse.py

writes tests/golden/contexttree_sparse_<case>.npz, one per case of tests/contexttree_sparse_oracle.py: CASES.  Trees are
stored as canonical node lists (level, symbols of the context, h_g, h_beta_vec, leaf; see the oracle's docstring), the
samples as uint8: data only.

Per case the fixture also records ``ref_vs_batch``, as make_golden_contexttree.py does: the largest
|dh_g| / (h_g (1 - h_g)) between the reference's sequential update and the sparse oracle's batch form over the update
stages.  ``map_stored`` = 0 marks the cases on which the reference's ``estimate_params(visualize=False)`` did not finish
within 30 s (it builds a full subtree under every missing node); they hold no MAP tree.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import contexttree                 # noqa: E402
import contexttree_sparse_oracle as sorc        # noqa: E402


def main():
    for case in sorc.CASES:
        inp = sorc.case_inputs(case)
        out, _ = sorc.drive(contexttree, case, inp)
        prior = sorc.stage_lists(out, "prior") if case["h0root"] else None
        ref_vs_batch = 0.0
        for stage, t in sorc.oracle_stages(case, inp, prior).items():
            ref = sorc.stage_lists(out, stage)
            assert sorc.same_node_set(t, ref), (case["name"], stage)
            assert np.array_equal(t["beta"], ref["beta"]) and np.array_equal(t["leaf"], ref["leaf"]), (case["name"], stage)
            ref_vs_batch = max(ref_vs_batch, sorc.g_err(t, ref))
        store = dict(out)
        for name in ("x1", "x2", "trace_x", "ctx0", "ctx1", "ctx2"):
            store[name] = inp[name].astype(np.uint8)
        store["ref_vs_batch"] = np.float64(ref_vs_batch)
        store["map_stored"] = np.uint8(case["map_stored"])
        path = os.path.join(HERE, f"contexttree_sparse_{case['name']}.npz")
        np.savez_compressed(path, **store)
        print(case["name"], "ref_vs_batch", ref_vs_batch, "nodes", len(out["after1_level"]),
              "deepest multi-sample node", int(out["after1_level"][out["after1_beta"].sum(1) > np.arange(
                  1, case["k"] + 1).sum() / 2.0 + 1].max(initial=-1)), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
