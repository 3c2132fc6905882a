"""ctypes binding of the fixed-posterior predictive engine of the context tree in ``libgmmvb.so`` (C ABI in
``include/ctpred.h``).

``PredPass`` borrows the tables of a ``_ctree.CtreePass`` or a ``_ctsp.SparseCtreePass`` in the form the model's store hands
them over (``contexttree._nodes``: ``beta, g, exists, off`` and, for hash tables, ``key``) and scores a held-out sample
under them: the row sums once per call, one scalar pass for ``ln p(x_i | context)``, one vector pass when the first maxima or
the full distributions are asked for, and a segmented sum per sequence.  Nothing is learnt and no table is written.  No CPU
fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._ctree import _CODES
from ._native import bind, stream_ptr

TILE = 256                               # include/ctpred.h: CTPRED_TILE
PIECE = 4096                             # include/ctpred.h: CTPRED_PIECE
UP_STACK, UP_PROBE = 0, 1                # enum ctpred_upwalk

_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_off = ctypes.POINTER(ctypes.c_int64)
# every symbol include/ctpred.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ctpred_abi_version": (_int, []),
    "ctpred_last_error": (ctypes.c_char_p, []),
    "ctpred_group_width": (_int, [_int]),
    "ctpred_rowsum_dense": (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "ctpred_rowsum_sparse": (_int, [_int, _int, _int, _off, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctpred_pass_dense": (_int, [_int, _vp, _i64, _vp, _i64, _int, _int, _int, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp,
                                 _vp, _vp]),
    "ctpred_pass_sparse": (_int, [_int, _vp, _i64, _vp, _i64, _int, _int, _int, _off, _vp, _vp, _vp, _vp, _vp, _dbl, _vp, _int,
                                  _vp, _vp, _vp, _vp, _vp]),
    "ctpred_plan_pieces": (_i64, [_off, _i64, _off]),
    "ctpred_totals": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
}

load_library, _check = bind("ctpred", SYMBOLS)


def group_width(k: int) -> int:
    """``ctpred_group_width`` in Python: W = min(64, 2^ceil(log2 k))."""
    return min(64, 1 << (int(k) - 1).bit_length())


def plan_pieces(seq_off):
    """``ctpred_plan_pieces`` in Python: the first piece of every sequence, and the piece count as the last element."""
    lens = np.diff(np.asarray(seq_off, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(-(-lens // PIECE))]).astype(np.int64)


def _ptr(t):
    return None if t is None else t.data_ptr()


class PredPass:
    """The entry points of ``include/ctpred.h`` on the tables of the engine ``eng``, read through ``store``."""

    upwalk = UP_STACK                    # the sparse up-walk (profiles/ctpred.md has the comparison)

    def __init__(self, eng, store):
        self.lib = load_library()
        self.eng, self.store = eng, store
        self.device = eng.device
        self.k, self.D = eng.k, eng.D
        assert self.lib.ctpred_group_width(self.k) == group_width(self.k)
        self._status = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.launch_info = ""

    def row_sums(self, t, has_tree: bool, hb: torch.Tensor) -> torch.Tensor:
        """``rowsum[slots + 1]`` of the tables ``t`` (enqueue only)."""
        slots = int(t["off"][-1])
        out = torch.empty(slots + 1, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            if "key" in t:
                off_c = (ctypes.c_int64 * (self.D + 2))(*t["off"])
                rc = self.lib.ctpred_rowsum_sparse(self.k, self.D, int(has_tree), off_c, t["key"].data_ptr(),
                                                   t["beta"].data_ptr(), t["exists"].data_ptr(), hb.data_ptr(),
                                                   out.data_ptr(), stream_ptr(self.device))
                _check(rc, "ctpred_rowsum_sparse")
            else:
                rc = self.lib.ctpred_rowsum_dense(self.k, self.D, int(has_tree), t["beta"].data_ptr(),
                                                  t["exists"].data_ptr(), hb.data_ptr(), out.data_ptr(),
                                                  stream_ptr(self.device))
                _check(rc, "ctpred_rowsum_dense")
        return out

    def passes(self, x, seq, t, has_tree, rowsum, hn_g, hb, lnp, arg, rows):
        """The scalar and / or the vector pass into the given outputs (enqueue only)."""
        n, S = int(x.shape[0]), 0 if seq is None else int(seq.shape[0]) - 1
        head = (_CODES[x.dtype], x.data_ptr(), n, _ptr(seq), S, self.k, self.D, int(has_tree))
        tail = (_ptr(lnp), _ptr(arg), _ptr(rows), self._status.data_ptr(), stream_ptr(self.device))
        with torch.cuda.device(self.device):
            if "key" in t:
                off_c = (ctypes.c_int64 * (self.D + 2))(*t["off"])
                rc = self.lib.ctpred_pass_sparse(*head, off_c, t["key"].data_ptr(), t["beta"].data_ptr(), t["g"].data_ptr(),
                                                 t["exists"].data_ptr(), rowsum.data_ptr(), float(hn_g), hb.data_ptr(),
                                                 int(self.upwalk), *tail)
                _check(rc, "ctpred_pass_sparse")
            else:
                rc = self.lib.ctpred_pass_dense(*head, t["beta"].data_ptr(), t["g"].data_ptr(), t["exists"].data_ptr(),
                                                rowsum.data_ptr(), float(hn_g), hb.data_ptr(), *tail)
                _check(rc, "ctpred_pass_dense")

    def totals(self, lnp, seq_off, seq):
        """Per-sequence sums of ``lnp``; ``seq_off`` on the host, ``seq`` the same on the device."""
        S = len(seq_off) - 1
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        piece_off = np.empty(S + 1, dtype=np.int64)
        pieces = int(self.lib.ctpred_plan_pieces(seq_off.ctypes.data_as(_off), S, piece_off.ctypes.data_as(_off)))
        assert pieces >= 0
        out = torch.empty(S, dtype=torch.float64, device=self.device)
        po = torch.as_tensor(piece_off, device=self.device) if pieces else None
        partial = torch.empty(pieces, dtype=torch.float64, device=self.device) if pieces else None
        with torch.cuda.device(self.device):
            rc = self.lib.ctpred_totals(lnp.data_ptr(), int(lnp.shape[0]), seq.data_ptr(), _ptr(po), S, pieces, _ptr(partial),
                                        out.data_ptr(), stream_ptr(self.device))
        _check(rc, "ctpred_totals")
        return out

    def run(self, x: torch.Tensor, seq_off, has_tree: bool, hn_g: float, hn_beta_vec, assign=False, dist=False, totals=False):
        """``x``: the adopted sample; ``seq_off``: S + 1 host int64 or None.  Returns ``(bad, lnp, z, rows, totals)``, device
        tensors (None where not asked for) after one host read of the status word; with ``bad > 0`` the rest means
        nothing."""
        dev, n = self.device, int(x.shape[0])
        t = self.store.pred_tables(self.eng)
        hb = torch.as_tensor(np.asarray(hn_beta_vec, dtype=np.float64), device=dev)
        seq = None if seq_off is None else torch.as_tensor(np.asarray(seq_off, dtype=np.int64), device=dev)
        rowsum = self.row_sums(t, has_tree, hb)
        lnp = torch.empty(n, dtype=torch.float64, device=dev)
        arg = torch.empty(n, dtype=torch.int64, device=dev) if assign else None
        rows = torch.empty(n, self.k, dtype=torch.float64, device=dev) if dist else None
        self.passes(x, seq, t, has_tree, rowsum, hn_g, hb, lnp, arg, rows)
        tot = self.totals(lnp, np.asarray(seq_off, dtype=np.int64), seq) if totals else None
        got_n, bad = (int(v) for v in self._status.cpu())
        assert got_n == n
        self.launch_info = ("ctpred_rowsum + ctpred_pass" + (" (scalar + vector)" if assign or dist else " (scalar)")
                            + (" + ctpred_totals" if totals else ""))
        return bad, lnp, arg, rows, tot
