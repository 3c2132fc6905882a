#!/usr/bin/env python3
"""Golden fixtures for contexttree, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_contexttree.py

writes tests/golden/contexttree_<case>.npz (one per case of tests/contexttree_oracle.py: CASES) and
contexttree_errors.json.  Trees are stored as dense per-level tables (g, beta, exists, leaf; see the oracle's docstring),
the samples as uint8.

Per case the fixture also records ``ref_vs_batch``: the largest |dh_g| / (h_g (1 - h_g)) between the reference's
sequential update and the oracle's batch form over the update stages (the log-odds error, so that values near 0 and near 1
are both held).  The GPU tests read their tolerance from it.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import contexttree          # noqa: E402
import contexttree_oracle as orc         # noqa: E402


def main():
    for case in orc.CASES:
        inp = orc.case_inputs(case)
        out, _ = orc.drive(contexttree, case, inp)
        ref_vs_batch = 0.0
        for stage, t in orc.oracle_stages(contexttree, case, inp).items():
            assert np.array_equal(t["beta"][t["exists"] != 0], out[f"{stage}_beta"][t["exists"] != 0]), (case["name"], stage)
            assert np.array_equal(t["exists"], out[f"{stage}_exists"]), (case["name"], stage)
            ref_vs_batch = max(ref_vs_batch, orc.log_odds_err(t["g"], out[f"{stage}_g"], t["exists"]))
        g = out["after1_g"][(out["after1_exists"] != 0) & (out["after1_g"] > 0)]
        store = {name: (a.astype(np.uint8) if name.endswith(("_exists", "_leaf", "_in_tree")) else a) for name, a in out.items()}
        for name in ("x1", "x2", "trace_x", "ctx0", "ctx1", "ctx2"):
            store[name] = inp[name].astype(np.uint8)
        store["ref_vs_batch"] = np.float64(ref_vs_batch)
        np.savez_compressed(os.path.join(HERE, f"contexttree_{case['name']}.npz"), **store)
        print(case["name"], "ref_vs_batch", ref_vs_batch, "min h_g", g.min() if g.size else None,
              "nodes", int(out["after1_exists"].sum()))
    errors = {name: orc.outcome(fn) for name, fn in orc.error_cases(contexttree).items()}
    with open(os.path.join(HERE, "contexttree_errors.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
    print(sum(v is not None for v in errors.values()), "of", len(errors), "boundary cases raise")


if __name__ == "__main__":
    main()
