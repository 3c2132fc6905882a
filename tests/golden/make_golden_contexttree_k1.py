#!/usr/bin/env python3
"""Golden fixture for contexttree at c_k = 1 with an absent child, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_contexttree_k1.py

writes tests/golden/contexttree_k1_absent_child.json: per case of ``contexttree_sparse_oracle.K1_CASES`` the posterior that
``set_hn_params(hn_root=...)`` leaves (canonical lists, see that module) and the outcome of ``estimate_params`` - its
canonical lists, or the exception class and message where the reference raises.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import contexttree          # noqa: E402
import contexttree_sparse_oracle as sorc  # noqa: E402


def main():
    out = {case["name"]: sorc.k1_drive(contexttree, case) for case in sorc.K1_CASES}
    with open(os.path.join(HERE, "contexttree_k1_absent_child.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for name, o in out.items():
        print(name, "nodes", len(o["posterior"]["level"]), "estimate_params:", o["map_outcome"] or "a tree")


if __name__ == "__main__":
    main()
