"""CPU stand-in for ``bayesml_amd._mtree.MtreePass`` (TEST INFRASTRUCTURE ONLY).

Implements the semantics of include/mtree.h with tests/metatree_oracle.py so that the HOST logic of ``metatree.LearnModel``
(type checks, refusal on ``bad``, flattening and materialising ``_Node`` forests, MTRF's copy of scikit-learn trees, the MAP
tree, pickle) can be tested without a GPU.  It is injected through the private ``LearnModel._mtree_pass_factory`` seam by
tests only; the product path never constructs it and fails loudly without the HIP engine.
"""
import numpy as np
import torch

import metatree_oracle as orc
from bayesml_amd import _expfam as xf
from bayesml_amd import _mtree


class CpuMtreePass:
    def __init__(self, flat, family, degree, dim_cont, dim_cat, cat_card, h0):
        _mtree.check_limits(flat.n_trees, flat.max_tree_nodes, flat.max_children, flat.max_depth, degree)
        self.flat, self.family, self.degree = flat.arrays(), int(family), int(degree)
        self.dim_cont, self.dim_cat = int(dim_cont), int(dim_cat)
        self.cat_card = np.asarray(cat_card, dtype=np.int64).reshape(-1)
        self.h0 = np.asarray(h0, dtype=np.float64)
        self.device = torch.device("cpu")
        self.state = None
        self.launch_info = "cpu stand-in"
        self.calls = []

    # the product's own dtype plumbing, so that the seam cannot hide what it does to the caller's values
    def adopt_x(self, x_continuous, x_categorical):
        xc = xf.adopt_tensor(x_continuous, self.device, "f", cols=self.dim_cont) if self.dim_cont else None
        xk = xf.adopt_tensor(x_categorical, self.device, "i", cols=self.dim_cat) if self.dim_cat else None
        return xc, xk

    def adopt_y(self, y):
        kind = "i" if self.family <= _mtree.POISSON else "f"
        return xf.adopt_tensor(y, self.device, kind).to(torch.int64 if kind == "i" else torch.float64)

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def update(self, xc, xk, y):
        xc, xk, y = self._np(xc), self._np(xk), y.numpy()
        n = len(y)
        self.calls.append(("update", n))
        bad = 0 if xk is None else int(((xk.astype(np.int64) < 0) | (xk.astype(np.int64) >= self.cat_card[None, :])).sum())
        if bad == 0:
            self.state, self.counts = orc.batch_update(self.flat, self.state, self.family, self.degree, self.h0,
                                                       self.dim_cont, xc, xk, y)
        return n, bad

    def predict(self, xc, xk, mode):
        name = {_mtree.PRED_MEAN: "mean", _mtree.PRED_PROBA: "proba", _mtree.PRED_CLASS: "class", _mtree.PRED_VAR: "var"}[mode]
        return orc.predict(self.flat, self.state, self.family, self.degree, self.dim_cont, self._np(xc), self._np(xk), name)

    def paths(self, xc, xk):
        return orc.route(self.flat, self.dim_cont, self._np(xc), self._np(xk))

    def get_state(self):
        return {k: np.array(v) for k, v in self.state.items()}

    def set_state(self, s):
        self.state = {k: np.array(s[k], dtype=np.float64) for k in orc.STATE}

    def close(self):
        pass


def use_cpu(cls_or_model):
    """Route a LearnModel (or the class) through the stand-in."""
    cls_or_model._mtree_pass_factory = staticmethod(CpuMtreePass) if isinstance(cls_or_model, type) else CpuMtreePass
    return cls_or_model
