"""ctypes binding of the sparse context-tree engine of ``libgmmvb.so`` (C ABI in ``include/ctsp.h``) over PyTorch-ROCm
tensors.

Where ``_ctree.CtreePass`` keeps a dense table per level, ``SparseCtreePass`` keeps one open-addressing hash table per level
that holds only the nodes that exist, so the shape is bounded by the key width (``bits(k) * D <= 63``) and by memory, not by
``k ** (D + 1)``.  A node is addressed by ``(level, key)``; ``key_of`` packs a context.  PyTorch owns the memory and the
stream and sizes the tables; count, level-up, sweep, MAP, lookup and growth are gfx950 kernels of ``csrc/ctsp_kernels.h``.
No CPU fallback: without the library or a GPU, ``SparseCtreePass`` raises ``EngineUnavailableError``.

Slot positions depend on which thread claimed a slot first; every read-out is therefore in canonical order (level, then
key), and only that order is deterministic.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._ctree import PassBase
from ._engine import EngineError, EngineLimitError
from ._native import bind, gpu_device, stream_ptr

U8, I32, I64 = range(3)                  # enum ctsp_dtype
MAX_K = 256                              # include/ctsp.h: CTSP_MAX_K
MAX_KEY_BITS = 63                        # include/ctsp.h: CTSP_MAX_KEY_BITS
EMPTY = -1                               # CTSP_EMPTY_KEY as the int64 that torch stores
# The default memory budget of one engine's tables: 64 GiB, under a quarter of the MI355X's 288 GB, so that a growth (old
# and new tables live together) and the sample still fit beside it.
DEFAULT_BUDGET = 64 << 30
DEFAULT_FLOOR = 64                       # smallest capacity of a level's table

_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_off = ctypes.POINTER(ctypes.c_int64)
# every symbol include/ctsp.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ctsp_abi_version": (_int, []),
    "ctsp_last_error": (ctypes.c_char_p, []),
    "ctsp_symbol_bits": (_int, [_int]),
    "ctsp_key_bits": (_int, [_int, _int]),
    "ctsp_capacity": (_i64, [_int, _int, _int, _i64, _i64, _i64]),
    "ctsp_slot_bytes": (_i64, [_int]),
    "ctsp_count": (_int, [_int, _vp, _i64, _int, _int, _off, _vp, _vp, _vp, _vp, _vp]),
    "ctsp_levelup": (_int, [_int, _int, _off, _vp, _vp, _vp, _int, _vp, _vp]),
    "ctsp_sweep": (_int, [_int, _int, _off, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _vp, _vp]),
    "ctsp_map": (_int, [_int, _int, _off, _vp, _vp, _vp, _dbl, _vp, _vp, _vp]),
    "ctsp_find": (_int, [_int, _int, _off, _vp, _i64, _vp, _vp, _int, _vp, _vp, _vp]),
    "ctsp_rehash": (_int, [_int, _int, _off, _vp, _vp, _vp, _vp, _vp, _off, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
_CODES = {torch.uint8: U8, torch.int32: I32, torch.int64: I64}

load_library, _check = bind("ctsp", SYMBOLS)


def symbol_bits(k: int) -> int:
    """b = max(1, ceil(log2 k))."""
    return max(1, (int(k) - 1).bit_length())


def check_limit(c_k: int, c_d_max: int):
    """Raised at model construction: a context must pack into 63 bits."""
    if c_k > MAX_K or symbol_bits(c_k) * c_d_max > MAX_KEY_BITS:
        raise EngineLimitError(f"bayesml_amd.contexttree with tables=\"sparse\" supports c_k <= {MAX_K} and "
                               f"ceil(log2 c_k) * c_d_max <= {MAX_KEY_BITS} in this version (got c_k = {c_k}, "
                               f"c_d_max = {c_d_max}); bayesml itself has no such limit")


def key_of(ctx, k: int, D: int) -> int:
    """The key of the context ``ctx`` = (x[i-1], x[i-2], ...), at most D symbols: level ``len(ctx)``."""
    b = symbol_bits(k)
    key = 0
    for j, c in enumerate(ctx):
        key |= int(c) << (b * (D - 1 - j))
    return key


def context_of(key: int, level: int, k: int, D: int):
    """The symbols (x[i-1], ..., x[i-level]) of a level-``level`` key."""
    b = symbol_bits(k)
    return [(int(key) >> (b * (D - 1 - j))) & ((1 << b) - 1) for j in range(level)]


def parent_key(key: int, level: int, k: int, D: int) -> int:
    """The level-(``level`` - 1) key above a level-``level`` key."""
    b = symbol_bits(k)
    return int(key) & ~((1 << (b * (D - level + 1))) - 1)


def child_key(key: int, level: int, c: int, k: int, D: int) -> int:
    """Child c of a level-``level`` key (level < D)."""
    return int(key) | (int(c) << (symbol_bits(k) * (D - level - 1)))


class SparseCtreePass(PassBase):
    """The hash tables of one context tree on one device and the entry points on them.

    ``budget_bytes``: the most the tables may take (``EngineLimitError`` beyond, state untouched).  ``floor_capacity``: the
    smallest capacity of a level (tests pass 2 to make every level grow).  ``growths`` counts the rehashes of a non-empty
    tree."""

    def __init__(self, k: int, D: int, device=None, *, budget_bytes: int = DEFAULT_BUDGET,
                 floor_capacity: int = DEFAULT_FLOOR):
        self.lib = load_library()
        check_limit(k, D)
        self.device = gpu_device(device, "sparse context-tree engine")
        self.k, self.D, self.b = int(k), int(D), symbol_bits(k)
        assert self.lib.ctsp_key_bits(self.k, self.D) == self.b * self.D
        self.budget_bytes, self.floor = int(budget_bytes), int(floor_capacity)
        self.slot_bytes = int(self.lib.ctsp_slot_bytes(self.k))
        self.growths = 0
        self.launch_info = ""
        self._status = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._used = [0] * (self.D + 1)         # upper bounds of the claimed slots per level
        self._alloc(self._plan([0] * (self.D + 1), 0))

    # ---- capacity ---------------------------------------------------------------------------------------------------------
    def _plan(self, present, n):
        """Capacities for ``present[d]`` claimed slots plus an update of n samples; never below the current ones."""
        caps = [int(self.lib.ctsp_capacity(self.k, self.D, d, int(present[d]), int(n), self.floor))
                for d in range(self.D + 1)]
        assert min(caps) >= 2
        if getattr(self, "caps", None):
            caps = [max(a, b) for a, b in zip(caps, self.caps)]
        return caps

    def _tables(self, caps):
        total = sum(caps)
        need = total * self.slot_bytes
        if need > self.budget_bytes:
            raise EngineLimitError(f"the sparse context-tree tables would take {need} bytes ({total} slots of "
                                   f"{self.slot_bytes} bytes at c_k = {self.k}; largest level {max(caps)} slots), above the "
                                   f"memory budget of {self.budget_bytes} bytes")
        if max(caps) > 1 << 30:
            raise EngineLimitError(f"a level of {max(caps)} slots is above the engine's 2**30 slots per level")
        dev = self.device
        return dict(key=torch.full((total,), EMPTY, dtype=torch.int64, device=dev),
                    beta=torch.zeros(total, self.k, dtype=torch.float64, device=dev),
                    g=torch.zeros(total, dtype=torch.float64, device=dev),
                    exists=torch.zeros(total, dtype=torch.uint8, device=dev),
                    leaf=torch.zeros(total, dtype=torch.uint8, device=dev),
                    cnt=torch.zeros(total, self.k, dtype=torch.int64, device=dev),
                    lnw=torch.zeros(total, dtype=torch.float64, device=dev))

    def _adopt_tables(self, caps, t):
        self.caps = list(caps)
        self.off = [0]
        for c in caps:
            self.off.append(self.off[-1] + c)
        self._off_c = (ctypes.c_int64 * (self.D + 2))(*self.off)
        self._off_t = torch.tensor(self.off, dtype=torch.int64, device=self.device)
        self.key, self.beta, self.g, self.exists, self.leaf = t["key"], t["beta"], t["g"], t["exists"], t["leaf"]
        self._cnt, self._lnw = t["cnt"], t["lnw"]

    def _alloc(self, caps):
        self._adopt_tables(caps, self._tables(caps))

    def _recount(self):
        """The claimed slots per level, exactly (one pass over the keys and one host read)."""
        c = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), (self.key != EMPTY).cumsum(0)])
        at = c[self._off_t].cpu().numpy()
        self._used = [int(v) for v in np.diff(at)]

    def _reserve(self, n, extra=None):
        """Room for an update of n samples (or ``extra[d]`` new nodes per level): grow by a rehash where the bound asks
        for it.  Raises ``EngineLimitError`` before anything changes."""
        def want():
            if extra is None:
                return self._plan(self._used, n)
            return self._plan([u + e for u, e in zip(self._used, extra)], 0)
        caps = want()
        if caps == self.caps:
            return
        self._recount()                 # the bound may only be loose
        caps = want()
        if caps == self.caps:
            return
        new = self._tables(caps)
        if any(self._used):
            old_off = self._off_c
            new_off = [0]
            for c in caps:
                new_off.append(new_off[-1] + c)
            new_off_c = (ctypes.c_int64 * (self.D + 2))(*new_off)
            with torch.cuda.device(self.device):
                rc = self.lib.ctsp_rehash(self.k, self.D, old_off, self.key.data_ptr(), self.beta.data_ptr(),
                                          self.g.data_ptr(), self.exists.data_ptr(), self.leaf.data_ptr(), new_off_c,
                                          new["key"].data_ptr(), new["beta"].data_ptr(), new["g"].data_ptr(),
                                          new["exists"].data_ptr(), new["leaf"].data_ptr(), self._status.data_ptr(),
                                          stream_ptr(self.device))
            _check(rc, "ctsp_rehash")
            self.growths += 1
            self.launch_info = "ctsp_rehash"
        self._adopt_tables(caps, new)
        if any(self._used):
            self._recount()             # (a rehash drops the slots that were claimed for a refused sample)

    # ---- the sample -------------------------------------------------------------------------------------------------------
    def count(self, x: torch.Tensor):
        """Zero the scratch and count the deepest level (enqueue only; the caller has reserved room)."""
        with torch.cuda.device(self.device):
            rc = self.lib.ctsp_count(_CODES[x.dtype], x.data_ptr(), x.shape[0], self.k, self.D, self._off_c,
                                     self.key.data_ptr(), self._cnt.data_ptr(), self._lnw.data_ptr(),
                                     self._status.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctsp_count")

    def levelup(self, x: torch.Tensor):
        head, n_head = self._head(x)
        with torch.cuda.device(self.device):
            rc = self.lib.ctsp_levelup(self.k, self.D, self._off_c, self.key.data_ptr(), self._cnt.data_ptr(),
                                       head.data_ptr() if n_head else None, n_head, self._status.data_ptr(),
                                       stream_ptr(self.device))
        _check(rc, "ctsp_levelup")

    def sweep(self, x: torch.Tensor, hn_g: float, hn_beta_vec):
        head, n_head = self._head(x)
        hb = torch.as_tensor(np.asarray(hn_beta_vec, dtype=np.float64), device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.ctsp_sweep(self.k, self.D, self._off_c, self.key.data_ptr(), self._cnt.data_ptr(),
                                     self._lnw.data_ptr(), self.beta.data_ptr(), self.g.data_ptr(), self.exists.data_ptr(),
                                     self.leaf.data_ptr(), head.data_ptr() if n_head else None, n_head, float(hn_g),
                                     hb.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctsp_sweep")

    def update(self, x, hn_g: float, hn_beta_vec):
        """reserve -> count -> level-up -> one host read of [n | bad | overflow] -> sweep unless bad > 0.  Returns
        (n, bad); with bad > 0 no node has changed."""
        n = int(x.shape[0])
        self._reserve(n)
        self.count(x)
        self.levelup(x)
        got_n, bad, overflow = (int(v) for v in self._status[:3].cpu())
        self._used = [min(u + min(n, self.k ** d), c) for d, (u, c) in enumerate(zip(self._used, self.caps))]
        if overflow:
            raise EngineError("ctsp: a hash table overflowed although it was sized from the upper bound; the posterior is "
                              "unchanged")
        if bad == 0:
            self.sweep(x, hn_g, hn_beta_vec)
        self.launch_info = "ctsp_count + ctsp_levelup" + (" + ctsp_sweep" if bad == 0 else "")
        return got_n, bad

    # ---- nodes by (level, key) ----------------------------------------------------------------------------------------------
    def find(self, levels, keys, insert=False) -> torch.Tensor:
        """Slot indices (int64 on the device, -1 = absent) of the nodes ``(levels[i], keys[i])``."""
        nq = len(levels)
        if nq == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        if insert:
            extra = np.bincount(np.asarray(levels, dtype=np.int64), minlength=self.D + 1)
            self._reserve(0, [int(v) for v in extra])
            self._used = [min(u + int(e), c) for u, e, c in zip(self._used, extra, self.caps)]
        ql = torch.as_tensor(np.asarray(levels, dtype=np.int32), device=self.device)
        qk = torch.as_tensor(np.asarray([int(v) for v in keys], dtype=np.uint64).view(np.int64), device=self.device)
        out = torch.empty(nq, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.ctsp_find(self.k, self.D, self._off_c, self.key.data_ptr(), nq, ql.data_ptr(), qk.data_ptr(),
                                    1 if insert else 0, out.data_ptr(), self._status.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctsp_find")
        return out

    def gather(self, path):
        """The nodes ``path`` (a short list of (level, key): one root-to-leaf path) as host arrays g, beta, exists, leaf;
        an absent node has exists = 0."""
        slot = self.find([p[0] for p in path], [p[1] for p in path])
        there = slot >= 0
        i = slot.clamp(min=0)
        ex = torch.where(there, self.exists[i], torch.zeros_like(self.exists[i]))
        return (self.g[i].cpu().numpy(), self.beta[i].cpu().numpy(), ex.cpu().numpy(), self.leaf[i].cpu().numpy())

    def scatter(self, path, g, beta, exists, leaf):
        slot = self.find([p[0] for p in path], [p[1] for p in path], insert=True)
        if bool((slot < 0).any()):
            raise EngineError("ctsp_find: a key does not belong to its level, or a table overflowed")
        self.g[slot] = torch.as_tensor(np.asarray(g, dtype=np.float64), device=self.device)
        self.beta[slot] = torch.as_tensor(np.asarray(beta, dtype=np.float64), device=self.device).reshape(len(path), self.k)
        self.exists[slot] = torch.as_tensor(np.asarray(exists, dtype=np.uint8), device=self.device)
        self.leaf[slot] = torch.as_tensor(np.asarray(leaf, dtype=np.uint8), device=self.device)

    def _node_slots(self):
        """Slot indices of the nodes in canonical order (level, then key), with their levels and keys, on the host."""
        idx = torch.nonzero((self.key != EMPTY) & (self.exists != 0)).reshape(-1)
        level = (torch.searchsorted(self._off_t, idx, right=True) - 1).cpu().numpy()
        key = self.key[idx].cpu().numpy()
        order = np.lexsort((key, level))
        return idx[torch.as_tensor(order, device=self.device)], level[order].astype(np.int32), key[order]

    def get_nodes(self):
        """Host arrays ``level, key, g, beta, leaf`` of every node, in canonical order."""
        idx, level, key = self._node_slots()
        return dict(level=level, key=key, g=self.g[idx].cpu().numpy(), beta=self.beta[idx].cpu().numpy(),
                    leaf=self.leaf[idx].cpu().numpy())

    def set_nodes(self, nodes):
        """Replace the tree by the given nodes (the arrays of ``get_nodes``)."""
        level = np.asarray(nodes["level"], dtype=np.int64)
        extra = [int(v) for v in np.bincount(level, minlength=self.D + 1)]
        caps = self._plan(extra, 0)
        if caps != self.caps:
            self._alloc_checked(caps)
        self.clear()
        if len(level):
            self.scatter(list(zip(level.tolist(), [int(v) for v in nodes["key"]])), nodes["g"], nodes["beta"],
                         np.ones(len(level), np.uint8), nodes["leaf"])

    def _alloc_checked(self, caps):
        new = self._tables(caps)        # raises before the old tables are let go
        self._adopt_tables(caps, new)

    def map_leaf(self, hn_g: float) -> np.ndarray:
        """map_leaf (uint8) of every node, in the canonical order of ``get_nodes``; the root must exist."""
        ml = torch.zeros(self.off[-1], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.ctsp_map(self.k, self.D, self._off_c, self.key.data_ptr(), self.g.data_ptr(),
                                   self.exists.data_ptr(), float(hn_g), self._lnw.data_ptr(), ml.data_ptr(),
                                   stream_ptr(self.device))
        _check(rc, "ctsp_map")
        self.launch_info = "ctsp_map"
        return ml[self._node_slots()[0]].cpu().numpy()

    def clear(self):
        self.key.fill_(EMPTY)
        self.exists.zero_()
        self.leaf.zero_()
        self._used = [0] * (self.D + 1)

    def close(self):
        self.key = self.beta = self.g = self.exists = self.leaf = self._cnt = self._lnw = None
