"""CPU stand-in for ``bayesml_amd._mtree.MtreePass`` with the linear-regression family (TEST INFRASTRUCTURE ONLY).

``fake_metatree_engine.CpuMtreePass`` with the update and the read-outs of tests/metatree_lr_oracle.py; every other family
goes to the parent class.  Injected through ``LearnModel._mtree_pass_factory`` by tests only.
"""
import metatree_lr_oracle as lro
from bayesml_amd import _mtree
from fake_metatree_engine import CpuMtreePass


class CpuMtreeLrPass(CpuMtreePass):
    def __init__(self, flat, family, degree, dim_cont, dim_cat, cat_card, h0):
        if family == _mtree.LINREG:
            _mtree.check_lr_degree(degree)
            super().__init__(flat, family, 0, dim_cont, dim_cat, cat_card, h0)
            self.degree = int(degree)
        else:
            super().__init__(flat, family, degree, dim_cont, dim_cat, cat_card, h0)

    def update(self, xc, xk, y):
        if self.family != _mtree.LINREG:
            return super().update(xc, xk, y)
        xc, xk, y = self._np(xc), self._np(xk), y.numpy()
        n = len(y)
        self.calls.append(("update", n))
        bad = 0 if xk is None else int(((xk < 0) | (xk >= self.cat_card[None, :])).sum())
        if bad == 0:
            self.state, self.counts, _ = lro.batch_update(self.flat, self.state, self.degree, self.h0, self.dim_cont, xc, xk, y)
        return n, bad

    def predict(self, xc, xk, mode):
        if self.family != _mtree.LINREG:
            return super().predict(xc, xk, mode)
        name = {_mtree.PRED_MEAN: "mean", _mtree.PRED_VAR: "var"}[mode]
        return lro.predict(self.flat, self.state, self.degree, self.dim_cont, self._np(xc), self._np(xk), name)


def use_cpu(cls_or_model):
    cls_or_model._mtree_pass_factory = staticmethod(CpuMtreeLrPass) if isinstance(cls_or_model, type) else CpuMtreeLrPass
    return cls_or_model
