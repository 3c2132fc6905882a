"""ctypes binding of the growth engine of ``libgmmvb.so`` (C ABI in ``include/mtgrow.h``) and the driver of one fit of
``metatree``'s MTMCMC / REMTMCMC over it.

A fit holds B chains.  Every chain's last tree and its proposal are complete C-ary trees of ``cap`` slots in heap order, so
one ``_mtree.MtreePass`` over the proposals' tables scores all B proposals with one ``mtree_route``, one ``mtree_reduce`` (or
``mtree_reduce_x``) and one ``mtree_sweep``.  ``Grower.step`` grows the proposals level by level (``mtgrow_level``), scores
them, and lets ``mtgrow_accept`` apply the test and copy the accepted tables over the last trees; the host reads back the
B x 4 buffer of that kernel, once per step.  The chain itself (the lists, the counts, g_max, the exchanges) is host code in
``bayesml_amd.metatree``.

Random numbers are addressed, not streamed: ``node_table`` and ``aux_table`` define every draw.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _mtree
from ._engine import EngineLimitError
from ._native import bind, stream_ptr

MIDPOINT, KMEANS = 0, 1                      # enum mtgrow_threshold
KMEANS_BLOCK = 1024                          # MTGROW_KMEANS_BLOCK
THRESHOLD = {"sample_midpoint": MIDPOINT, "1d_kmeans": KMEANS}

_vp, _i64, _i32, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_double


class StateStruct(ctypes.Structure):
    """struct mtgrow_state."""
    _fields_ = ([(k, _i32) for k in ("n_chains", "cap", "n_children", "dim_cont", "dim_cat", "max_depth", "n_post", "threshold")]
                + [("n", _i64), ("xc_dtype", _i32), ("xk_dtype", _i32)]
                + [(k, _vp) for k in ("xc_dev", "xk_dev", "order_dev", "draws_dev", "last_feat_dev", "last_g_dev", "feat_dev",
                                      "thr_dev", "g_dev", "post_dev", "node_dev", "open_dev", "regen_dev", "dflag_dev",
                                      "first_dev", "count_dev", "differs_dev", "lo_dev", "hi_dev", "mid_dev")])


_sp = ctypes.POINTER(StateStruct)
# every symbol include/mtgrow.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mtgrow_abi_version": (_int, []),
    "mtgrow_last_error": (ctypes.c_char_p, []),
    "mtgrow_capacity": (_i64, [_int, _int]),
    "mtgrow_begin": (_int, [_sp, _dbl, _dbl, _vp, _vp]),
    "mtgrow_level": (_int, [_sp, _int, _int, _dbl, _vp]),
    "mtgrow_accept": (_int, [_sp, _int, _dbl] + [_vp] * 14),
}

load_library, _check = bind("mtgrow", SYMBOLS)


def node_table(seed, t: int, n_chains: int, cap: int) -> np.ndarray:
    """[B, cap, 2] draws of step t: slot h of chain b tests keep / flip with [b, h, 0] and draws its feature with [b, h, 1].
    The step is the third word of the Philox counter (the generator counts its blocks in the first word, so tables at
    consecutive first words would share all but four of their values)."""
    return np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, t, 0])).random((n_chains, cap, 2))


def aux_table(seed, t: int, n_chains: int, num_exchange: int = 0) -> np.ndarray:
    """[B + 2 num_exchange] draws of step t: the chains' acceptance draws, then per exchange attempt e the pair draw
    (j = floor(u (B - 1))) at [B + 2 e] and the test draw at [B + 2 e + 1]."""
    return np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, t, 1])).random(n_chains + 2 * num_exchange)


def fresh_key() -> int:
    """A Philox key from fresh entropy (``seed=None``)."""
    return int(np.random.SeedSequence().generate_state(1, np.uint64)[0])


def capacity(n_children: int, max_depth: int, n_chains: int = 1) -> int:
    """Slots of a chain's complete tree; the engine's tables are sized by it (the reference has no such limit)."""
    cap = (n_children ** (max_depth + 1) - 1) // (n_children - 1)
    if cap > _mtree.MAX_NODES or n_chains > _mtree.MAX_TREES or max_depth > _mtree.MAX_DEPTH:
        raise EngineLimitError(
            f"bayesml_amd.metatree grows MTMCMC / REMTMCMC proposals in complete trees of at most {_mtree.MAX_NODES} nodes "
            f"((C^(c_max_depth + 1) - 1) / (C - 1)) for at most {_mtree.MAX_TREES} chains in this version (got {cap} nodes, "
            f"{n_chains} chains); bayesml itself has no such limit")
    return cap


def complete_forest(n_chains: int, n_children: int, max_depth: int) -> _mtree.FlatForest:
    """The static tables of B complete C-ary trees in heap order; ``feat`` (all leaves) and ``thr`` are what growth writes."""
    C, cap = n_children, capacity(n_children, max_depth, n_chains)
    depth = np.zeros(cap, dtype=np.int32)
    for h in range(1, cap):
        depth[h] = depth[(h - 1) // C] + 1
    h = np.arange(cap, dtype=np.int64)
    inner = depth < max_depth
    B = n_chains
    base = (np.arange(B, dtype=np.int64) * cap)[:, None]
    child0 = np.where(inner[None, :], base + C * h[None, :] + 1, 0)
    return _mtree.FlatForest(
        tree_off=(np.arange(B + 1, dtype=np.int64) * cap).astype(np.int32), feat=np.full(B * cap, -1, dtype=np.int32),
        child0=child0.reshape(-1).astype(np.int32), nchild=np.tile(np.where(inner, C, 0), B).astype(np.int32),
        thr_off=(np.arange(B * cap, dtype=np.int64) * (C + 1)).astype(np.int32), depth=np.tile(depth, B),
        thr=np.zeros(B * cap * (C + 1)))


class Grower:
    """The device side of one fit: B chains over one sample."""

    def __init__(self, family, degree, dim_cont, dim_cat, cat_card, n_children, max_depth, h0, sub_hn, g_root, g_below,
                 threshold_type, n_chains, xc, xk, y, device=None):
        self.lib = load_library()
        self.B, self.C, self.max_depth = int(n_chains), int(n_children), int(max_depth)
        self.cap = capacity(self.C, self.max_depth, self.B)
        self.g_root, self.g_below = float(g_root), float(g_below)
        self.eng = eng = _mtree.MtreePass(complete_forest(self.B, self.C, self.max_depth), family, degree, dim_cont, dim_cat,
                                          cat_card, h0, device=device)
        self.device = dev = eng.device
        self.xc, self.xk = eng.adopt_x(xc, xk)
        self.y = eng.adopt_y(y)
        self.n = int(self.y.shape[0])
        if self.n >= 2 ** 31:
            raise EngineLimitError(f"bayesml_amd.metatree: an MTMCMC / REMTMCMC fit takes at most 2^31 - 1 rows (got {self.n}); "
                                   "bayesml itself has no such limit")
        B, cap, C, P = self.B, self.cap, self.C, eng.np_
        self.threshold = THRESHOLD[threshold_type]
        self.order = None
        if self.threshold == KMEANS and C == 2 and dim_cont > 0:       # every feature's order, once per fit
            self.order = torch.sort(self.xc.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous()
        self.sub_hn = torch.zeros(P, dtype=torch.float64, device=dev)
        sub_hn = np.asarray(sub_hn, dtype=np.float64).reshape(-1)
        self.sub_hn[:len(sub_hn)] = torch.from_numpy(sub_hn)

        def table(dtype, *shape):
            return torch.zeros(*shape, dtype=dtype, device=dev)
        self.draws = table(torch.float64, B, cap, 2)
        self.last = dict(feat=torch.full((B * cap,), -1, dtype=torch.int32, device=dev), thr=table(torch.float64, B * cap * (C + 1)),
                         g=table(torch.float64, B * cap), post=table(torch.float64, B * cap, P),
                         lml=table(torch.float64, B * cap), lcm=table(torch.float64, B * cap))
        self.node = table(torch.int32, B, self.n)
        self._slots = {k: table(torch.int32, B * cap) for k in ("open", "regen", "dflag", "first", "count", "differs")}
        self._lo, self._hi = table(torch.int64, B * cap), table(torch.int64, B * cap)
        self._mid = table(torch.float64, B * cap)
        self.l_new, self.l_last = table(torch.float64, B), table(torch.float64, B)
        self._beta, self._u, self._out = table(torch.float64, B), table(torch.float64, B), table(torch.float64, B, 4)
        cc, ck = eng._codes(self.xc, self.xk)
        p = _mtree._ptr
        self.struct = StateStruct(B, cap, C, eng.dim_cont, eng.dim_cat, self.max_depth, P, self.threshold, self.n, cc, ck,
                                  p(self.xc), p(self.xk), p(self.order), p(self.draws), p(self.last["feat"]), p(self.last["g"]),
                                  p(eng._tabs["feat"]), p(eng._tabs["thr"]), p(eng.g), p(eng.post), p(self.node),
                                  *(p(self._slots[k]) for k in ("open", "regen", "dflag", "first", "count", "differs")),
                                  p(self._lo), p(self._hi), p(self._mid))
        self.launch_info = ""

    # ---- one proposal per chain ---------------------------------------------------------------------------------------------
    def grow(self, draws, all_regen, g_max, levels=None):
        """Grows the B proposals from ``draws`` [B, cap, 2] (host); enqueue only."""
        self.draws.copy_(torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float64)), non_blocking=False)
        ref, q = ctypes.byref(self.struct), stream_ptr(self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.mtgrow_begin(ref, self.g_root, self.g_below, self.sub_hn.data_ptr(), q), "mtgrow_begin")
            for d in range(self.max_depth if levels is None else levels):
                _check(self.lib.mtgrow_level(ref, d, int(all_regen), float(g_max), q), "mtgrow_level")

    def score(self):
        """route -> reduce -> sweep over the proposals: l_new[b] = L of chain b's root.  Returns ``bad`` (device)."""
        eng = self.eng
        stop, _, bad = eng.route(self.xc, self.xk)
        if eng.family == _mtree.LINREG:
            eng.reduce_x(stop, self.xc, self.y)
        else:
            eng.reduce(stop, self.y)
        work = eng._scratch(1)
        eng.lml.fill_(float("nan"))
        eng.lcm.zero_()
        self.l_new.zero_()
        with torch.cuda.device(self.device):
            rc = self.lib.mtree_sweep(ctypes.byref(eng.struct), eng.family, eng.degree, eng.stat_int.data_ptr(),
                                      eng.stat_real.data_ptr(), eng.h0.data_ptr(), eng.post.data_ptr(), eng.g.data_ptr(),
                                      eng.lml.data_ptr(), eng.lcm.data_ptr(), self.l_new.data_ptr(), work.data_ptr(),
                                      stream_ptr(self.device))
        _mtree._check(rc, "mtree_sweep")
        self.launch_info = f"mtgrow_level x {self.max_depth} + mtree_route + mtree_reduce + mtree_sweep + mtgrow_accept"
        return stop, bad

    def start(self, draws):
        """The chains' initial trees (every node regenerated).  Returns (l_last[B], bad)."""
        self.grow(draws, True, 0.0)
        _, bad = self.score()
        self.last["feat"].copy_(self.eng._tabs["feat"])
        self.last["thr"].copy_(self.eng._tabs["thr"])
        self.last["g"].copy_(self.eng.g)
        self.last["post"].copy_(self.eng.post)
        self.last["lml"].copy_(self.eng.lml)
        self.last["lcm"].copy_(self.eng.lcm)
        self.l_last.copy_(self.l_new)
        return self.l_last.cpu().numpy(), int(bad.cpu()[0])

    def step(self, draws, u_accept, beta, g_max):
        """One Metropolis-Hastings step of every chain; ``beta`` None is the untempered test of MTMCMC.  Returns the host
        array [B, 4] = (accepted, l_new, tp_new, tp_last), the step's only read-back."""
        self.grow(draws, False, g_max)
        self.score()
        self._u.copy_(torch.from_numpy(np.ascontiguousarray(u_accept, dtype=np.float64)))
        if beta is not None:
            self._beta.copy_(torch.from_numpy(np.ascontiguousarray(beta, dtype=np.float64)))
        L = self.last
        with torch.cuda.device(self.device):
            rc = self.lib.mtgrow_accept(ctypes.byref(self.struct), int(beta is not None), float(g_max), self.l_new.data_ptr(),
                                        self.l_last.data_ptr(), self._beta.data_ptr(), self._u.data_ptr(), self.eng.lml.data_ptr(),
                                        self.eng.lcm.data_ptr(), L["feat"].data_ptr(), L["thr"].data_ptr(), L["g"].data_ptr(),
                                        L["post"].data_ptr(), L["lml"].data_ptr(), L["lcm"].data_ptr(), self._out.data_ptr(),
                                        stream_ptr(self.device))
        _check(rc, "mtgrow_accept")
        return self._out.cpu().numpy()

    def swap(self, j):
        """Exchanges the last trees of chains j and j + 1: their table slices and l_last."""
        cap, C = self.cap, self.C
        for name, width in (("feat", 1), ("thr", C + 1), ("g", 1), ("lml", 1), ("lcm", 1)):
            t = self.last[name].view(self.B, cap * width)
            t[[j, j + 1]] = t[[j + 1, j]]
        self.last["post"].view(self.B, cap, -1)[[j, j + 1]] = self.last["post"].view(self.B, cap, -1)[[j + 1, j]]
        self.l_last[[j, j + 1]] = self.l_last[[j + 1, j]]

    def snapshot(self, b):
        """Chain b's last tree as host tables: feat[cap], thr[cap, C + 1], g[cap], post[cap, P], lml[cap], lcm[cap]."""
        cap, C = self.cap, self.C
        return dict(feat=self.last["feat"].view(self.B, cap)[b].cpu().numpy().astype(np.int64),
                    thr=self.last["thr"].view(self.B, cap, C + 1)[b].cpu().numpy(),
                    g=self.last["g"].view(self.B, cap)[b].cpu().numpy(), post=self.last["post"].view(self.B, cap, -1)[b].cpu().numpy(),
                    lml=self.last["lml"].view(self.B, cap)[b].cpu().numpy(), lcm=self.last["lcm"].view(self.B, cap)[b].cpu().numpy())

    def proposal(self):
        """The proposals' tables and the growth scratch on the host, for tests."""
        B, cap, C = self.B, self.cap, self.C
        out = {k: v.view(B, cap).cpu().numpy() for k, v in self._slots.items()}
        out.update(feat=self.eng._tabs["feat"].view(B, cap).cpu().numpy(), thr=self.eng._tabs["thr"].view(B, cap, C + 1).cpu().numpy(),
                   g=self.eng.g.view(B, cap).cpu().numpy(), post=self.eng.post.view(B, cap, -1).cpu().numpy(),
                   node=self.node.cpu().numpy(), l_new=self.l_new.cpu().numpy())
        return out

    def close(self):
        self.eng.close()
