"""CPU stand-ins for ``bayesml_amd._ctree.CtreePass`` and ``bayesml_amd._ctsp.SparseCtreePass`` (TEST INFRASTRUCTURE ONLY).

Implement the semantics of include/ctree.h in NumPy (tests/contexttree_oracle.py), and of include/ctsp.h on a node
dictionary (tests/contexttree_sparse_oracle.py), so that the HOST logic of
``contexttree.LearnModel`` (type checks, refusal on ``bad``, tree scatter and materialisation, path work, pickle) can be
tested without a GPU.  They are injected through the private ``LearnModel._ctree_pass_factory`` seam by tests only; the product
path never constructs them and fails loudly without the HIP engine.
"""
import numpy as np
import torch

import contexttree_oracle as orc
import contexttree_sparse_oracle as sorc
from bayesml_amd import _expfam as xf


class CpuCtreePass:
    def __init__(self, k, D):
        self.k, self.D, self.off = int(k), int(D), orc.offsets(k, D)
        self.nodes = self.off[-1]
        self.t = orc.new_tables(k, D)
        self.device = torch.device("cpu")
        self.launch_info = "cpu stand-in"
        self.calls = []

    def adopt(self, x):
        # the product's own dtype plumbing, so that the seam cannot hide what it does to the caller's values
        return xf.adopt_tensor(x, self.device, "i")

    def any_negative(self, x):
        return bool((x.to(torch.int64) < 0).any())

    def update(self, x, hn_g, hn_beta_vec):
        assert x.dtype in (torch.uint8, torch.int32, torch.int64) and x.dim() == 1 and x.shape[0] >= 1
        self.calls.append(("update", str(x.dtype), int(x.shape[0])))
        v = x.to(torch.int64).numpy()
        bad = int(((v < 0) | (v >= self.k)).sum())
        if bad == 0:
            orc.batch_update(v, self.k, self.D, self.t, hn_g, hn_beta_vec)
        return len(v), bad

    def map_leaf(self, hn_g):
        assert self.t["exists"][0]
        return orc.map_tables(self.k, self.D, self.t, hn_g)

    def get_tables(self):
        return orc.copy_tables(self.t)

    def set_tables(self, t):
        self.t = {name: np.array(t[name], dtype=self.t[name].dtype) for name in ("g", "beta", "exists", "leaf")}

    def clear(self):
        self.t["exists"][:] = 0
        self.t["leaf"][:] = 0

    def fill_existing(self, g=None, beta=None):
        m = self.t["exists"] != 0
        if g is not None:
            self.t["g"][m] = g
            self.t["g"][self.off[self.D]:][m[self.off[self.D]:]] = 0.0
        if beta is not None:
            self.t["beta"][m] = np.asarray(beta, dtype=float)

    def gather(self, idx):
        i = np.asarray(list(idx), dtype=np.int64)
        return self.t["g"][i], self.t["beta"][i], self.t["exists"][i], self.t["leaf"][i]

    def scatter(self, idx, g, beta, exists, leaf):
        i = np.asarray(list(idx), dtype=np.int64)
        self.t["g"][i], self.t["beta"][i] = np.asarray(g, dtype=float), np.asarray(beta, dtype=float)
        self.t["exists"][i], self.t["leaf"][i] = np.asarray(exists, np.uint8), np.asarray(leaf, np.uint8)

    def close(self):
        pass


class CpuSparseCtreePass:
    """Nodes by (level, key) in a dict ``{(level, key): [g, beta, leaf]}``; every read-out in canonical order."""

    def __init__(self, k, D):
        self.k, self.D, self.nd = int(k), int(D), {}
        self.device = torch.device("cpu")
        self.launch_info = "cpu stand-in"

    adopt, any_negative = CpuCtreePass.adopt, CpuCtreePass.any_negative

    def update(self, x, hn_g, hn_beta_vec):
        assert x.dtype in (torch.uint8, torch.int32, torch.int64) and x.dim() == 1 and x.shape[0] >= 1
        v = x.to(torch.int64).numpy()
        bad = int(((v < 0) | (v >= self.k)).sum())
        if bad == 0:
            sorc.batch_update(v, self.k, self.D, self.nd, hn_g, hn_beta_vec)
        return len(v), bad

    def map_leaf(self, hn_g):
        ml = sorc.map_nodes(self.k, self.D, self.nd, hn_g)
        return np.array([ml[at] for at in sorted(self.nd)], dtype=np.uint8)

    def get_nodes(self):
        order = sorted(self.nd)
        return dict(level=np.array([d for d, _ in order], dtype=np.int32), key=np.array([s for _, s in order], dtype=np.int64),
                    g=np.array([self.nd[at][0] for at in order], dtype=np.float64),
                    beta=np.array([self.nd[at][1] for at in order], dtype=np.float64).reshape(len(order), self.k),
                    leaf=np.array([self.nd[at][2] for at in order], dtype=np.uint8))

    def set_nodes(self, nodes):
        self.clear()
        self.scatter(list(zip(nodes["level"], nodes["key"])), nodes["g"], nodes["beta"], np.ones(len(nodes["g"])), nodes["leaf"])

    def clear(self):
        self.nd = {}

    def fill_existing(self, g=None, beta=None):
        for (d, _), row in self.nd.items():
            if g is not None:
                row[0] = 0.0 if d == self.D else float(g)
            if beta is not None:
                row[1] = np.array(beta, dtype=float)

    def gather(self, path):
        rows = [self.nd.get((int(d), int(s))) for d, s in path]
        return (np.array([r[0] if r else 0.0 for r in rows]),
                np.array([r[1] if r else np.zeros(self.k) for r in rows]).reshape(len(rows), self.k),
                np.array([r is not None for r in rows], dtype=np.uint8), np.array([r[2] if r else 0 for r in rows], np.uint8))

    def scatter(self, path, g, beta, exists, leaf):
        assert all(0 <= d <= self.D and 0 <= int(s) < 1 << (sorc.bits(self.k) * self.D) for d, s in path) and np.all(exists)
        beta = np.asarray(beta, dtype=float).reshape(len(path), self.k)
        for (d, s), g_, b_, lf in zip(path, g, beta, leaf):
            self.nd[(int(d), int(s))] = [float(g_), b_.copy(), int(lf)]

    def close(self):
        pass


def use_cpu(cls_or_model):
    """Route a LearnModel (or, for constructors that need the tables, the class) through the dense stand-in."""
    cls_or_model._ctree_pass_factory = staticmethod(CpuCtreePass) if isinstance(cls_or_model, type) else CpuCtreePass
    return cls_or_model
