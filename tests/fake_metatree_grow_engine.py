"""CPU stand-in for ``bayesml_amd._mtgrow.Grower`` (TEST INFRASTRUCTURE ONLY): ``fake_metatree_engine.CpuMtreePass`` plus the
growth capability, from tests/metatree_mcmc_oracle.py with the addressed draw tables the model hands over.  It lets the HOST
side of MTMCMC / REMTMCMC (the preconditions, the lists and counts, g_max, the exchanges, the stdout protocol, the merge and
the installed forest) be tested without a GPU.  Injected through ``LearnModel._mtree_pass_factory`` by tests only.
"""
import numpy as np
import torch

import metatree_mcmc_oracle as mc
from bayesml_amd import _expfam as xf
from bayesml_amd import _mtree
from fake_metatree_engine import CpuMtreePass

KEYS = ("feat", "thr", "g", "post", "lml", "lcm")


class CpuGrower:
    def __init__(self, family, degree, dim_cont, dim_cat, cat_card, n_children, max_depth, h0, sub_hn, g_root, g_below,
                 threshold_type, n_chains, xc, xk, y):
        self.cfg = mc.Config(family, degree, dim_cont, dim_cat, n_children, max_depth, h0, sub_hn, g_root, g_below,
                             threshold_type)
        self.B, self.cap = int(n_chains), self.cfg.cap
        dev = torch.device("cpu")
        self.xc = xf.adopt_tensor(xc, dev, "f", cols=dim_cont) if dim_cont else None
        self.xk = xf.adopt_tensor(xk, dev, "i", cols=dim_cat) if dim_cat else None
        kind = "i" if family <= _mtree.POISSON else "f"
        self.y = xf.adopt_tensor(y, dev, kind).to(torch.int64 if kind == "i" else torch.float64).numpy()
        self._xc = None if self.xc is None else self.xc.numpy()
        self._xk = None if self.xk is None else self.xk.numpy()
        self.cat_card = np.asarray(cat_card, dtype=np.int64).reshape(-1)
        self.last, self.l_last = [None] * self.B, np.zeros(self.B)
        self.steps = 0

    def _tables(self, T):
        """The oracle's tables in the engine's form: lcm[c] = the L the parent took for child c."""
        out = {k: np.array(T[k]) for k in ("feat", "thr", "g", "post", "lml")}
        out["lcm"] = np.array(T.get("lcm", np.zeros(self.cap)))
        return out

    def _grow(self, draws, b, last, g_max):
        return mc.grow(self.cfg, self._xc, self._xk, self.y, draws, b, last, g_max)

    def start(self, draws):
        bad = 0 if self._xk is None else int(((self._xk < 0) | (self._xk >= self.cat_card[None, :])).sum())
        if bad:
            return self.l_last, bad
        d = mc.TableDraws(draws, None, self.B)
        for b in range(self.B):
            self.last[b] = self._grow(d, b, None, 0.0)
            self.l_last[b] = self.last[b]["L"]
        return self.l_last.copy(), 0

    def step(self, draws, u_accept, beta, g_max):
        self.steps += 1
        d = mc.TableDraws(draws, np.asarray(u_accept), self.B)
        out = np.zeros((self.B, 4))
        for b in range(self.B):
            new = self._grow(d, b, self.last[b], g_max)
            tp_new = mc.truncated_posterior(self.cfg, new, new["dflag"], g_max)
            tp_last = mc.truncated_posterior(self.cfg, self.last[b], new["dflag"], g_max)
            if beta is None:
                a = np.exp(new["L"] - tp_last - self.l_last[b] + tp_new)
            else:
                a = np.exp((new["L"] - self.l_last[b]) * beta[b] - tp_last + tp_new)
            ok = u_accept[b] < a
            out[b] = (ok, new["L"], tp_new, tp_last)
            if ok:
                self.last[b], self.l_last[b] = new, new["L"]
        return out

    def swap(self, j):
        self.last[j], self.last[j + 1] = self.last[j + 1], self.last[j]
        self.l_last[[j, j + 1]] = self.l_last[[j + 1, j]]

    def snapshot(self, b):
        return self._tables(self.last[b])

    def close(self):
        pass


class CpuMtreeGrowPass(CpuMtreePass):
    grower = CpuGrower


def use_cpu(cls_or_model):
    """Route a LearnModel (or the class) through the stand-in with growth."""
    cls_or_model._mtree_pass_factory = staticmethod(CpuMtreeGrowPass) if isinstance(cls_or_model, type) else CpuMtreeGrowPass
    return cls_or_model
