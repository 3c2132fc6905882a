"""ctypes binding of the sequential context-tree engine of ``libgmmvb.so`` (C ABI in ``include/ctseq.h``).

``SequencePass`` borrows the dense tables of a ``_ctree.CtreePass`` and runs ``ctseq_pass`` over a sample chunk by chunk:
every position's predictive distribution before its symbol is seen, then the update by it, as n calls of
``LearnModel.pred_and_update`` would do, in one group of launches per level and chunk.  Chunks run strictly in order and
carry state only through the tables, so the chunk length changes the workspace and nothing else about a chunk's own
arithmetic.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._ctree import _CODES
from ._native import bind, stream_ptr

TILE = 256                               # include/ctseq.h: CTSEQ_TILE
ROW_BLOCK = 64                           # include/ctseq.h: CTSEQ_ROW_BLOCK
DEFAULT_CHUNK_BYTES = 256 << 20
MAX_M = (1 << 31) - 1

_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
# every symbol include/ctseq.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ctseq_abi_version": (_int, []),
    "ctseq_last_error": (ctypes.c_char_p, []),
    "ctseq_work_len": (_i64, [_int, _int, _i64, _int]),
    "ctseq_pass": (_int, [_int, _vp, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("ctseq", SYMBOLS)


def work_slots(k: int, D: int, m: int, want_rows: bool) -> int:
    """``ctseq_work_len`` in Python (csrc/ctseq.hip: layout_of), so that chunks can be planned without the library."""
    h, tiles = (m + 1) // 2, (m + TILE - 1) // TILE
    return ((m * k if want_rows else 0) + 2 * h * (D + 1) + 4 * h + 6 * m + ((k + 1) * tiles + 1) // 2 + 2 * tiles
            + (tiles + 1) // 2 + (m + D + 7) // 8)


def plan_chunks(n: int, k: int, D: int, want_rows: bool, chunk_bytes=None) -> int:
    """The chunk length m: the largest 1 <= m <= min(n, 2^31 - 1) whose workspace fits ``chunk_bytes`` (m = 1 if none
    does).  ``want_rows``: the workspace holds an [m][k] row buffer (asked for by loss "0-1")."""
    budget = DEFAULT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    lo, hi = 1, max(1, min(int(n), MAX_M))
    while lo < hi:                        # work_slots grows strictly with m
        mid = (lo + hi + 1) // 2
        if 8 * work_slots(k, D, mid, want_rows) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo


class SequencePass:
    """``ctseq_pass`` over a whole sample on the tables of the ``CtreePass`` ``eng``."""

    def __init__(self, eng):
        self.lib = load_library()
        self.eng = eng
        self.device = eng.device
        self.launch_info = ""
        self.passes = 0

    def run(self, x: torch.Tensor, hn_g: float, hn_beta_vec, want, want_nats: bool, chunk_bytes=None):
        """``want``: "rows", "argmax" or None.  Returns (prediction or None, nats or None, last row or None), device
        tensors; the loop enqueues only."""
        eng, dev = self.eng, self.device
        n, k, D = int(x.shape[0]), eng.k, eng.D
        inner = want == "argmax"
        m = plan_chunks(n, k, D, inner, chunk_bytes)
        slots = int(self.lib.ctseq_work_len(k, D, m, int(inner)))
        assert slots == work_slots(k, D, m, inner)
        work = torch.empty(slots, dtype=torch.int64, device=dev)
        rows = torch.empty(n, k, dtype=torch.float64, device=dev) if want == "rows" else None
        arg = torch.empty(n, dtype=torch.int64, device=dev) if inner else None
        nats = torch.empty(n, dtype=torch.float64, device=dev) if want_nats else None
        hb = torch.as_tensor(np.asarray(hn_beta_vec, dtype=np.float64), device=dev)
        self.passes = 0
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            for begin in range(0, n, m):
                mm = min(m, n - begin)
                rc = self.lib.ctseq_pass(_CODES[x.dtype], x.data_ptr(), n, begin, mm, k, D, eng.beta.data_ptr(),
                                         eng.g.data_ptr(), eng.exists.data_ptr(), eng.leaf.data_ptr(), float(hn_g),
                                         hb.data_ptr(), rows[begin:].data_ptr() if rows is not None else None,
                                         arg[begin:].data_ptr() if inner else None,
                                         nats[begin:].data_ptr() if want_nats else None, work.data_ptr(), stream)
                _check(rc, "ctseq_pass")
                self.passes += 1
        last = None
        if rows is not None:
            last = rows[n - 1]
        elif inner:                       # the row buffer of the last pass lies at the start of the workspace
            last = work[(mm - 1) * k:mm * k].view(torch.float64)
        self.launch_info = f"ctseq_pass x {self.passes} (m = {m})"
        return (rows if rows is not None else arg), nats, last
