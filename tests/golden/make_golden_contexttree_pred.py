#!/usr/bin/env python3
"""Golden fixtures for ``contexttree.LearnModel.calc_pred_logpdf``, produced by the REFERENCE (build container only):

    MPLBACKEND=Agg python tests/golden/make_golden_contexttree_pred.py

writes tests/golden/contexttree_pred_<case>.npz, one per case of tests/contexttree_oracle.py: CASES (dense) and of
tests/contexttree_sparse_oracle.py: CASES (``sparse_<case>``).  Each case is driven to its final model as the existing
fixtures were (and its tree is checked against what they store), then a seeded held-out sample ``y`` with ``lengths``
(``contexttree_pred_oracle.heldout``) is scored position by position with the reference's ``calc_pred_dist(y_s[:i + 1])``:
``p_one`` [n, k] takes ``y`` as one sequence, ``p_split`` [n, k] as the sequences of ``lengths``.  ``hn_g`` and
``hn_beta_vec`` are the final model's defaults.  The sparse cases also store their final tree as canonical node lists
(``final_level``, ``final_ctx``, ``final_g``, ``final_beta``, ``final_leaf``), which the existing sparse fixtures do not
hold.  Data only.
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import contexttree                 # noqa: E402
import contexttree_oracle as orc                # noqa: E402
import contexttree_pred_oracle as porc          # noqa: E402
import contexttree_sparse_oracle as sorc        # noqa: E402


def load(name):
    with np.load(os.path.join(HERE, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def score(m, y, lengths):
    """The reference's p_theta_vec after calc_pred_dist(y_s[:i + 1]) for every position of every sequence."""
    mc = copy.deepcopy(m)
    at = np.concatenate([[0], np.cumsum(lengths)])
    rows = np.zeros((len(y), m.c_k))
    for a, b in zip(at[:-1], at[1:]):
        ys = y[a:b]
        for i in range(len(ys)):
            rows[a + i] = mc.calc_pred_dist(ys[:i + 1]).p_theta_vec
    return rows


def main():
    for sparse, mod in ((False, orc), (True, sorc)):
        for case in mod.CASES:
            k, D = case["k"], case["D"]
            inp = mod.case_inputs(case)
            out, m = mod.drive(contexttree, case, inp)
            name = ("sparse_" if sparse else "") + case["name"]
            old = load(f"contexttree_{name}.npz")
            store = {}
            if sparse:
                assert int(old["final_nodes"]) == len(sorc.tree_to_nodes(m.hn_root, k, D)), name
                assert np.array_equal(old["trace_p"], out["trace_p"]), name
                for key, a in sorc.tree_to_lists(m.hn_root, k, D).items():
                    store[f"final_{key}"] = a
                get = porc.sparse_lookup(sorc.tree_to_nodes(m.hn_root, k, D), k, D)
            else:
                t = orc.tree_to_tables(m.hn_root, k, D)
                for key in ("g", "beta", "exists", "leaf"):
                    assert np.array_equal(old[f"final_{key}"], t[key]), (name, key)
                get = porc.dense_lookup(t, k, D)
            y, lengths = porc.heldout(case, inp["x1"])
            store.update(y=y.astype(np.uint8), lengths=lengths, p_one=score(m, y, np.array([len(y)])),
                         p_split=score(m, y, lengths), hn_g=np.float64(m.hn_g), hn_beta_vec=np.array(m.hn_beta_vec))
            # the restatement, here already: it must sit inside the bound before a fixture is written
            for rows, ln in ((store["p_one"], None), (store["p_split"], lengths)):
                mine = porc.pred_rows(y, ln, k, D, get, m.hn_g, m.hn_beta_vec)
                assert np.all(np.abs(mine - rows) <= porc.p_rel_reference(k, D) * rows), name
            unclear = 1.0 - min(porc.z_clear(store["p_one"], k, D).mean(), porc.z_clear(store["p_split"], k, D).mean())
            assert unclear <= 0.02, (name, unclear)
            path = os.path.join(HERE, f"contexttree_pred_{name}.npz")
            np.savez_compressed(path, **store)
            print(name, "n", len(y), "positions without a clear maximum", unclear, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
