"""ctypes binding of the context-tree engine of ``libgmmvb.so`` (C ABI in ``include/ctree.h``) over PyTorch-ROCm tensors.

The division of labour is ``_expfam``'s: PyTorch owns device memory and the stream; the pass over the sample that counts
every (context, symbol) pair and the per-level sweeps over the tree are gfx950 kernels of ``csrc/ctree_kernels.h``; what
touches one root-to-leaf path or one node tree is host code in ``bayesml_amd.contexttree``.  No CPU fallback: without the
library or a GPU, ``CtreePass`` raises ``EngineUnavailableError``.

The tree lives in dense tables over all levels (level d starts at ``off[d]``, keys in order; the key of the context
``(x[i-1], ..., x[i-d])`` is ``sum_j x[i-j] k^(j-1)`` and child c of key s has key ``s + c k^d``): ``g[nodes]`` and
``beta[nodes, k]`` float64, ``exists[nodes]`` and ``leaf[nodes]`` uint8.  A node with ``exists = 0`` has not been created
yet; its other entries mean nothing.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._engine import EngineLimitError
from ._native import PLOT_MSG, bind, gpu_device, stream_ptr  # noqa: F401  (PLOT_MSG: the model package reads it here)
from ._expfam import adopt_tensor

U8, I32, I64 = range(3)                  # enum ctree_dtype
MAX_K = 256                              # include/ctree.h: CTREE_MAX_K
MAX_SLOTS = 1 << 24                      # include/ctree.h: CTREE_MAX_SLOTS

_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
# every symbol include/ctree.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ctree_abi_version": (_int, []),
    "ctree_last_error": (ctypes.c_char_p, []),
    "ctree_table_len": (_i64, [_int, _int, _int]),
    "ctree_work_len": (_i64, [_int, _int]),
    "ctree_count": (_int, [_int, _vp, _i64, _int, _int, _vp, _vp, _vp]),
    "ctree_sweep": (_int, [_int, _int, _vp, _vp, _int, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp]),
    "ctree_map": (_int, [_int, _int, _vp, _vp, _dbl, _vp, _vp, _vp]),
}
_CODES = {torch.uint8: U8, torch.int32: I32, torch.int64: I64}

load_library, _check = bind("ctree", SYMBOLS)


def check_limit(c_k: int, c_d_max: int):
    """Raised at model construction: the deepest count table has k^(D+1) slots (the reference has no such limit; the
    sparse tables of ``_ctsp`` are opt-in, ``LearnModel(..., tables="sparse")``)."""
    if c_k > MAX_K or c_k ** (c_d_max + 1) > MAX_SLOTS or c_d_max > 24:
        raise EngineLimitError(f"bayesml_amd.contexttree supports c_k <= {MAX_K} and c_k ** (c_d_max + 1) <= {MAX_SLOTS} in "
                               f"this version (got c_k = {c_k}, c_d_max = {c_d_max}); bayesml itself has no such limit, and "
                               f"tables=\"sparse\" goes to ceil(log2 c_k) * c_d_max <= 63")


def offsets(k: int, D: int):
    """First entry of every level in an all-levels table, and the entry count as the last element."""
    off = [0]
    for d in range(D + 1):
        off.append(off[-1] + k ** d)
    return off


class PassBase:
    """What ``CtreePass`` and ``_ctsp.SparseCtreePass`` spell alike: nothing here depends on how a level's table is laid
    out, only on ``device``, ``D``, ``off`` (level D is the last) and the tensors ``g``, ``beta`` and ``exists``."""

    def adopt(self, x):
        return adopt_tensor(x, self.device, "i")

    def any_negative(self, x) -> bool:
        return bool((x < 0).any()) if x.dtype != torch.uint8 else False

    def _head(self, x):
        """The first min(n, D) symbols as int32, and their number: the samples that end above the maximal depth."""
        n_head = min(int(x.shape[0]), self.D)
        return x[:n_head].to(torch.int32), n_head

    def fill_existing(self, g=None, beta=None):
        """What the reference's ``_set_hn_g_recursion`` / ``_set_hn_beta_vec_recursion`` do: every existing node gets the
        value (g = 0 at the maximal depth)."""
        m = self.exists != 0
        if g is not None:
            oD = self.off[self.D]
            self.g[:oD] = torch.where(m[:oD], float(g), self.g[:oD])
            self.g[oD:] = torch.where(m[oD:], 0.0, self.g[oD:])
        if beta is not None:
            b = torch.as_tensor(np.asarray(beta, dtype=np.float64), device=self.device)
            self.beta.copy_(torch.where(m[:, None], b[None, :], self.beta))


class CtreePass(PassBase):
    """The tables of one context tree on one device and the three entry points on them."""

    def __init__(self, k: int, D: int, device=None):
        self.lib = load_library()
        check_limit(k, D)
        self.device = gpu_device(device, "context-tree engine")
        self.k, self.D, self.off = int(k), int(D), offsets(k, D)
        self.nodes = self.off[-1]
        assert self.nodes == self.lib.ctree_table_len(self.k, self.D, -1)
        dev = self.device
        self.g = torch.zeros(self.nodes, dtype=torch.float64, device=dev)
        self.beta = torch.zeros(self.nodes, self.k, dtype=torch.float64, device=dev)
        self.exists = torch.zeros(self.nodes, dtype=torch.uint8, device=dev)
        self.leaf = torch.zeros(self.nodes, dtype=torch.uint8, device=dev)
        self._work = torch.empty(int(self.lib.ctree_work_len(self.k, self.D)), dtype=torch.int64, device=dev)
        self._out = torch.empty(2 + self.k ** (self.D + 1), dtype=torch.int64, device=dev)
        self.launch_info = ""

    # ---- the sample -----------------------------------------------------------------------------------------------------
    def count(self, x: torch.Tensor) -> torch.Tensor:
        """``[n | bad | cnt_D[k^D][k]]`` of the adopted sample, int64 on the device (overwritten by the next call)."""
        with torch.cuda.device(self.device):
            rc = self.lib.ctree_count(_CODES[x.dtype], x.data_ptr(), x.shape[0], self.k, self.D, self._out.data_ptr(),
                                      self._work.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctree_count")
        self.launch_info = "ctree_count"
        return self._out

    def sweep(self, x: torch.Tensor, hn_g: float, hn_beta_vec, want_counts=False):
        """The up-sweep on the counts of the last ``count(x)``.  With ``want_counts`` the counts of levels 0..D-1 are
        returned as an int64 tensor [nodes of those levels, k]."""
        head, n_head = self._head(x)
        hb = torch.as_tensor(np.asarray(hn_beta_vec, dtype=np.float64), device=self.device)
        cl = torch.zeros(self.off[self.D], self.k, dtype=torch.int64, device=self.device) if want_counts else None
        with torch.cuda.device(self.device):
            rc = self.lib.ctree_sweep(self.k, self.D, self._out.data_ptr() + 16, head.data_ptr(), n_head, self.beta.data_ptr(),
                                      self.g.data_ptr(), self.exists.data_ptr(), float(hn_g), hb.data_ptr(),
                                      cl.data_ptr() if want_counts else None, self._work.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctree_sweep")
        oD = self.off[self.D]
        self.leaf[oD:] = self.exists[oD:]         # a node at the maximal depth is a leaf from its creation on
        self.launch_info = "ctree_count + ctree_sweep"
        return cl

    def update(self, x, hn_g: float, hn_beta_vec):
        """count -> one host read of [n | bad] -> sweep unless bad > 0.  Returns (n, bad); with bad > 0 nothing changed."""
        n, bad = (int(v) for v in self.count(x)[:2].cpu())
        if bad == 0:
            self.sweep(x, hn_g, hn_beta_vec)
        return n, bad

    def map_leaf(self, hn_g: float) -> np.ndarray:
        """The map_leaf table (uint8, all levels) of the current state; the root must exist."""
        ml = torch.empty(self.nodes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.ctree_map(self.k, self.D, self.g.data_ptr(), self.exists.data_ptr(), float(hn_g), ml.data_ptr(),
                                    self._work.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctree_map")
        self.launch_info = "ctree_map"
        return ml.cpu().numpy()

    # ---- the tables -----------------------------------------------------------------------------------------------------
    def get_tables(self):
        return dict(g=self.g.cpu().numpy(), beta=self.beta.cpu().numpy(), exists=self.exists.cpu().numpy(),
                    leaf=self.leaf.cpu().numpy())

    def set_tables(self, t):
        for name in ("g", "beta", "exists", "leaf"):
            getattr(self, name).copy_(torch.from_numpy(np.ascontiguousarray(t[name])))

    def clear(self):
        self.exists.zero_()
        self.leaf.zero_()

    def gather(self, idx):
        """The rows ``idx`` (a short list of table indices: one path) as host arrays g, beta, exists, leaf."""
        i = torch.as_tensor(list(idx), dtype=torch.int64, device=self.device)
        return (self.g[i].cpu().numpy(), self.beta[i].cpu().numpy(), self.exists[i].cpu().numpy(), self.leaf[i].cpu().numpy())

    def scatter(self, idx, g, beta, exists, leaf):
        i = torch.as_tensor(list(idx), dtype=torch.int64, device=self.device)
        self.g[i] = torch.as_tensor(np.asarray(g, dtype=np.float64), device=self.device)
        self.beta[i] = torch.as_tensor(np.asarray(beta, dtype=np.float64), device=self.device)
        self.exists[i] = torch.as_tensor(np.asarray(exists, dtype=np.uint8), device=self.device)
        self.leaf[i] = torch.as_tensor(np.asarray(leaf, dtype=np.uint8), device=self.device)

    def close(self):
        self._work = self._out = None

