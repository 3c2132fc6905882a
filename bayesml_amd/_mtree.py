"""ctypes binding of the meta-tree forest engine of ``libgmmvb.so`` (C ABI in ``include/mtree.h``) over PyTorch-ROCm tensors.

The division of labour is ``_ctree``'s: PyTorch owns device memory and the stream; routing every row through every tree, the
segmented reduction of y, the bottom-up sweep and the predictive fold are gfx950 kernels of ``csrc/mtree_kernels.h``; what
touches one node tree (materialising ``_Node`` objects, the MAP tree, feature importances) is host code in
``bayesml_amd.metatree``.  No CPU fallback: without the library or a GPU, ``MtreePass`` raises ``EngineUnavailableError``.
The linear-regression family (``LINREG``, kernels in ``csrc/mtree_lr_kernels.h``) reduces x as well: ``reduce_x`` hands the
feature matrix to ``mtree_reduce_x``, and the predictive table is sized by ``mtree_values_len``.

The forest lives in flat tables over all trees (``FlatForest``): ``tree_off[B + 1]``, and per node ``feat`` (-1 for a leaf),
``child0``, ``nchild``, ``thr_off``, ``depth``, nodes of a tree in breadth-first order; the state is ``g[nodes]``,
``post[nodes, P]`` (the family's posterior vector), ``lml[nodes]`` (NaN where a node was never visited), ``lcm[nodes]`` (the L its parent last took for a node) and ``prob[B]``,
all float64.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from ._engine import EngineLimitError
from ._native import PLOT_MSG, bind, gpu_device, stream_ptr  # noqa: F401  (PLOT_MSG: the model package reads it here)
from ._expfam import adopt_tensor

U8, I32, I64, F32, F64 = range(5)                                  # enum mtree_dtype
BERNOULLI, CATEGORICAL, POISSON, EXPONENTIAL, NORMAL, LINREG = range(6)    # enum mtree_family
PRED_MEAN, PRED_PROBA, PRED_CLASS, PRED_VAR = range(4)             # enum mtree_pred
MAX_TREES, MAX_NODES, MAX_CHILDREN, MAX_DEGREE, MAX_DEPTH, MAX_SLABS = 1024, 4096, 16, 16, 24, 64    # include/mtree.h
LDS_SLOTS = 6144
LR_MAX_DEGREE, LR_BLOCK = 15, 1024          # MTREE_LR_MAX_DEGREE, MTREE_LR_BLOCK
MIN_SPAN = 1024              # a wave is given at least this many rows of a tree
WORK_SLOTS = 1 << 26         # the slabs of one reduction stay below this many 8-byte slots (512 MiB)

_vp, _i64, _i32, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int
_ip = ctypes.POINTER(ctypes.c_int)


class ForestStruct(ctypes.Structure):
    """struct mtree_forest."""
    _fields_ = [("n_trees", _i32), ("n_nodes", _i32), ("n_thr", _i32), ("max_tree_nodes", _i32), ("max_children", _i32),
                ("max_depth", _i32), ("dim_cont", _i32), ("dim_cat", _i32), ("tree_off_dev", _vp), ("feat_dev", _vp),
                ("child0_dev", _vp), ("nchild_dev", _vp), ("thr_off_dev", _vp), ("depth_dev", _vp), ("thr_dev", _vp)]


_fp = ctypes.POINTER(ForestStruct)
# every symbol include/mtree.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mtree_abi_version": (_int, []),
    "mtree_last_error": (ctypes.c_char_p, []),
    "mtree_stat_cols": (_int, [_int, _int, _ip, _ip, _ip]),
    "mtree_work_len": (_i64, [_i32, _int, _int, _int]),
    "mtree_route": (_int, [_fp, _int, _vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mtree_reduce": (_int, [_fp, _int, _int, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mtree_reduce_x_work_len": (_i64, [_i32, _i32, _int, _i64, _int]),
    "mtree_reduce_x": (_int, [_fp, _int, _int, _vp, _int, _vp, _i64, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "mtree_values_len": (_i64, [_i32, _int, _int]),
    "mtree_sweep": (_int, [_fp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mtree_predict": (_int, [_fp, _int, _int, _int, _int, _vp, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}
_CODES = {torch.uint8: U8, torch.int32: I32, torch.int64: I64, torch.float32: F32, torch.float64: F64}

load_library, _check = bind("mtree", SYMBOLS)


def stat_cols(family: int, degree: int = 0):
    """(int64 columns, float64 columns, length of the posterior vector) of a family: include/mtree.h, mtree_stat_cols."""
    tri = degree * (degree + 1) // 2
    return {BERNOULLI: (2, 0, 2), CATEGORICAL: (1 + degree, 0, degree), POISSON: (2, 1, 3), EXPONENTIAL: (1, 1, 2),
            NORMAL: (1, 3, 5), LINREG: (1, tri + degree + 1, degree + tri + 3)}[family]


def check_lr_degree(degree: int):
    """The linear-regression sub-model's regressors and y share one 16-column MFMA tile (include/mtree.h)."""
    if degree > LR_MAX_DEGREE:
        raise EngineLimitError(
            f"bayesml_amd.metatree supports SubModel=linearregression up to c_degree = {LR_MAX_DEGREE} in this version "
            f"(got {degree}); bayesml itself has no such limit")


@dataclass
class FlatForest:
    """The structure tables of a forest as host arrays (int32 but ``thr``, float64)."""
    tree_off: np.ndarray
    feat: np.ndarray
    child0: np.ndarray
    nchild: np.ndarray
    thr_off: np.ndarray
    depth: np.ndarray
    thr: np.ndarray

    @property
    def n_trees(self):
        return len(self.tree_off) - 1

    @property
    def n_nodes(self):
        return len(self.feat)

    @property
    def max_tree_nodes(self):
        return int(np.diff(self.tree_off).max())

    @property
    def max_children(self):
        return int(self.nchild.max()) if self.n_nodes else 0

    @property
    def max_depth(self):
        return int(self.depth.max())

    def arrays(self):
        return {name: getattr(self, name) for name in ("tree_off", "feat", "child0", "nchild", "thr_off", "depth", "thr")}


def check_limits(n_trees: int, max_tree_nodes: int, max_children: int, max_depth: int, degree: int = 0):
    """Raised where a forest is handed to the engine: its tables are sized by these bounds (the reference has none)."""
    if (n_trees > MAX_TREES or max_tree_nodes > MAX_NODES or max_children > MAX_CHILDREN or max_depth > MAX_DEPTH
            or degree > MAX_DEGREE):
        raise EngineLimitError(
            f"bayesml_amd.metatree supports at most {MAX_TREES} trees, {MAX_NODES} nodes per tree, {MAX_CHILDREN} children per "
            f"node, depth {MAX_DEPTH} and a categorical degree of {MAX_DEGREE} in this version (got {n_trees} trees, "
            f"{max_tree_nodes} nodes in the largest tree, {max_children} children, depth {max_depth}, degree {degree}); "
            "bayesml itself has no such limit")


def slabs_for(n: int, n_nodes: int, cols: int) -> int:
    """Row slabs of one reduction: one per MIN_SPAN rows, at most MAX_SLABS, and scratch below WORK_SLOTS."""
    assert n >= 1 and n_nodes >= 1 and cols >= 1
    return int(max(1, min(MAX_SLABS, -(-n // MIN_SPAN), WORK_SLOTS // max(1, n_nodes * cols))))


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


class MtreePass:
    """The tables of one forest on one device and the entry points on them."""

    def __init__(self, flat: FlatForest, family: int, degree: int, dim_cont: int, dim_cat: int, cat_card, h0, device=None):
        self.lib = load_library()
        check_limits(flat.n_trees, flat.max_tree_nodes, flat.max_children, flat.max_depth, 0 if family == LINREG else degree)
        if family == LINREG:
            check_lr_degree(degree)
        self.device = gpu_device(device, "meta-tree engine")
        self.flat, self.family, self.degree = flat, int(family), int(degree)
        self.dim_cont, self.dim_cat = int(dim_cont), int(dim_cat)
        self.ni, self.nr, self.np_ = stat_cols(self.family, self.degree)
        dev = self.device
        self._tabs = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64 if k == "thr" else np.int32)).to(dev)
                      for k, v in flat.arrays().items()}
        self.cat_card = torch.as_tensor(np.asarray(cat_card, dtype=np.int32).reshape(-1), device=dev)
        self.h0 = torch.zeros(self.np_, dtype=torch.float64, device=dev)
        h0 = np.asarray(h0, dtype=np.float64).reshape(-1)
        self.h0[:len(h0)] = torch.from_numpy(h0)
        nodes, B = flat.n_nodes, flat.n_trees
        self.g = torch.zeros(nodes, dtype=torch.float64, device=dev)
        self.post = torch.zeros(nodes, self.np_, dtype=torch.float64, device=dev)
        self.lml = torch.full((nodes,), float("nan"), dtype=torch.float64, device=dev)
        self.lcm = torch.zeros(nodes, dtype=torch.float64, device=dev)
        self.prob = torch.full((B,), 1.0 / B, dtype=torch.float64, device=dev)
        self.stat_int = torch.zeros(nodes, self.ni, dtype=torch.int64, device=dev)
        self.stat_real = torch.zeros(nodes, max(1, self.nr), dtype=torch.float64, device=dev)
        self._values = torch.empty(int(self.lib.mtree_values_len(nodes, self.family, self.degree)), dtype=torch.float64,
                                   device=dev)
        self._bad = torch.zeros(1, dtype=torch.int64, device=dev)
        self._work = self._work_x = None
        self.struct = ForestStruct(B, nodes, len(flat.thr), flat.max_tree_nodes, flat.max_children, flat.max_depth,
                                   self.dim_cont, self.dim_cat, *(_ptr(self._tabs[k]) for k in
                                                                  ("tree_off", "feat", "child0", "nchild", "thr_off", "depth", "thr")))
        self.launch_info = ""

    # ---- the sample -----------------------------------------------------------------------------------------------------
    def adopt_x(self, x_continuous, x_categorical):
        """The feature matrices as [n, dim] tensors on the device in a dtype the kernels read (None where dim = 0)."""
        xc = adopt_tensor(x_continuous, self.device, "f", cols=self.dim_cont) if self.dim_cont else None
        xk = adopt_tensor(x_categorical, self.device, "i", cols=self.dim_cat) if self.dim_cat else None
        if xc is not None and not xc.is_contiguous():
            xc = xc.contiguous()
        if xk is not None and not xk.is_contiguous():
            xk = xk.contiguous()
        return xc, xk

    def adopt_y(self, y):
        """y as int64 (discrete families) or float64 on the device."""
        kind = "i" if self.family <= POISSON else "f"
        t = adopt_tensor(y, self.device, kind)
        return t.to(torch.int64 if kind == "i" else torch.float64)

    @staticmethod
    def _codes(xc, xk):
        return (_CODES[xc.dtype] if xc is not None else F64), (_CODES[xk.dtype] if xk is not None else U8)

    def route(self, xc, xk, want_path=False):
        """(stop[B, n], path[B, n, max_depth + 1] or None, bad) -- bad stays on the device."""
        n = int((xc if xc is not None else xk).shape[0])
        B = self.flat.n_trees
        stop = torch.empty(B, n, dtype=torch.int32, device=self.device)
        path = torch.empty(B, n, self.flat.max_depth + 1, dtype=torch.int32, device=self.device) if want_path else None
        cc, ck = self._codes(xc, xk)
        with torch.cuda.device(self.device):
            rc = self.lib.mtree_route(ctypes.byref(self.struct), cc, _ptr(xc), ck, _ptr(xk), _ptr(self.cat_card), n,
                                      stop.data_ptr(), _ptr(path), self._bad.data_ptr(), stream_ptr(self.device))
        _check(rc, "mtree_route")
        return stop, path, self._bad

    def _scratch(self, S):
        need = int(self.lib.mtree_work_len(self.flat.n_nodes, self.family, self.degree, S))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.int64, device=self.device)
        return self._work

    def reduce_x(self, stop, x, y):
        """The reduction of a family whose statistics need x (LINREG): x is [n, >= degree], read with its row stride."""
        n = int(stop.shape[1])
        S = slabs_for(n, self.flat.n_nodes, 1)
        need = int(self.lib.mtree_reduce_x_work_len(self.flat.n_nodes, self.flat.n_trees, self.degree, n, S))
        if need < 0:
            raise EngineLimitError(f"bayesml_amd.metatree: a linear-regression update takes at most 2^31 - 1 rows (got {n}); "
                                   "bayesml itself has no such limit")
        if self._work_x is None or self._work_x.numel() < need:
            self._work_x = None
            self._work_x = torch.empty(need, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.mtree_reduce_x(ctypes.byref(self.struct), self.family, self.degree, stop.data_ptr(), _CODES[x.dtype],
                                         x.data_ptr(), int(x.stride(0)), y.data_ptr(), n, S, self.stat_int.data_ptr(),
                                         self.stat_real.data_ptr(), self._work_x.data_ptr(), stream_ptr(self.device))
        _check(rc, "mtree_reduce_x")

    def reduce(self, stop, y):
        n = int(stop.shape[1])
        S = slabs_for(n, self.flat.n_nodes, self.ni + min(self.nr, 1))
        work = self._scratch(S)
        with torch.cuda.device(self.device):
            rc = self.lib.mtree_reduce(ctypes.byref(self.struct), self.family, self.degree, stop.data_ptr(), y.data_ptr(),
                                       n, S, self.stat_int.data_ptr(), self.stat_real.data_ptr(), work.data_ptr(),
                                       stream_ptr(self.device))
        _check(rc, "mtree_reduce")

    def sweep(self):
        work = self._scratch(1)
        lnp = torch.log(self.prob)
        with torch.cuda.device(self.device):
            rc = self.lib.mtree_sweep(ctypes.byref(self.struct), self.family, self.degree, self.stat_int.data_ptr(),
                                      self.stat_real.data_ptr(), self.h0.data_ptr(), self.post.data_ptr(),
                                      self.g.data_ptr(), self.lml.data_ptr(), self.lcm.data_ptr(), lnp.data_ptr(), work.data_ptr(),
                                      stream_ptr(self.device))
        _check(rc, "mtree_sweep")
        p = torch.exp(lnp - lnp.max())
        self.prob.copy_(p / p.sum())

    def update(self, xc, xk, y):
        """route -> one host read of ``bad`` -> reduce -> sweep.  Returns (n, bad); with bad > 0 nothing changed."""
        stop, _, bad = self.route(xc, xk)
        n, bad = int(stop.shape[1]), int(bad.cpu()[0])
        if bad == 0:
            if self.family == LINREG:
                self.reduce_x(stop, xc, y)
            else:
                self.reduce(stop, y)
            self.sweep()
            self.launch_info = f"mtree_route + mtree_reduce{'_x' if self.family == LINREG else ''} + mtree_sweep"
        return n, bad

    def predict(self, xc, xk, mode):
        n = int((xc if xc is not None else xk).shape[0])
        C = 2 if self.family == BERNOULLI else self.degree if self.family == CATEGORICAL else 1
        if mode == PRED_CLASS:
            out = torch.empty(n, dtype=torch.int64, device=self.device)
        else:
            out = torch.empty((n, C) if mode == PRED_PROBA else (n,), dtype=torch.float64, device=self.device)
        cc, ck = self._codes(xc, xk)
        with torch.cuda.device(self.device):
            rc = self.lib.mtree_predict(ctypes.byref(self.struct), self.family, self.degree, mode, cc, _ptr(xc), ck, _ptr(xk),
                                        n, self.post.data_ptr(), self.g.data_ptr(), self.prob.data_ptr(),
                                        self._values.data_ptr(), out.data_ptr(), stream_ptr(self.device))
        _check(rc, "mtree_predict")
        self.launch_info = "mtree_predict"
        return out.cpu().numpy()

    def paths(self, xc, xk):
        """The walks as a host array [B, n, max_depth + 1] of table indices, -1 past the stop node."""
        return self.route(xc, xk, want_path=True)[1].cpu().numpy()

    # ---- the tables -----------------------------------------------------------------------------------------------------
    def get_state(self):
        return dict(g=self.g.cpu().numpy(), post=self.post.cpu().numpy(), lml=self.lml.cpu().numpy(),
                    lcm=self.lcm.cpu().numpy(), prob=self.prob.cpu().numpy())

    def set_state(self, s):
        for name in ("g", "post", "lml", "lcm", "prob"):
            getattr(self, name).copy_(torch.from_numpy(np.ascontiguousarray(s[name], dtype=np.float64)))

    def last_stats(self):
        """The statistics tables after the last update (subtree totals; normal: mu, c, SS of include/mtree.h), for tests."""
        return self.stat_int.cpu().numpy(), self.stat_real.cpu().numpy()[:, :self.nr]

    def close(self):
        self._work = self._work_x = None

