"""ctypes binding of the many-sequence fit of the context tree in ``libgmmvb.so`` (C ABI in ``include/ctfit.h``).

``FitPass`` borrows the dense tables of a ``_ctree.CtreePass`` and applies the update that the loop
``for s in seqs: update_posterior(s)`` leaves, in one device pass: the segmented count and the head records, the two
orderings of the heads (``torch.sort`` of packed 64-bit keys), the ranks and lead of every node with heads, and the sweep
with lead.  The host builds only the S + 1 offsets ``seq_off`` and ``hoff``; ``[n | bad]`` is read once, after the count,
and the tables are first written after it.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._ctree import _CODES
from ._native import bind, stream_ptr

TILE = 256                               # include/ctfit.h: CTFIT_TILE
SEQ_STAGE = 512                          # include/ctfit.h: CTFIT_SEQ_STAGE
SERIAL_RUN = 32                          # include/ctfit.h: CTFIT_SERIAL_RUN

_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
# every symbol include/ctfit.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ctfit_abi_version": (_int, []),
    "ctfit_last_error": (ctypes.c_char_p, []),
    "ctfit_work_len": (_i64, [_int, _int]),
    "ctfit_head_len": (_i64, [_i64]),
    "ctfit_count": (_int, [_int, _vp, _i64, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    "ctfit_rank": (_int, [_int, _vp, _i64, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctfit_sweep": (_int, [_int, _int, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _vp]),
}

load_library, _check = bind("ctfit", SYMBOLS)


def head_offsets(seq_off, D: int) -> np.ndarray:
    """``hoff``: the exclusive prefix of min(len_s, D), S + 1 int64; the last element is the number of heads."""
    lens = np.diff(np.asarray(seq_off, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(np.minimum(lens, D))]).astype(np.int64)


class FitPass:
    """The entry points of ``include/ctfit.h`` on the tables of the dense engine ``eng``."""

    def __init__(self, eng):
        self.lib = load_library()
        self.eng = eng
        self.device = eng.device
        self.k, self.D = eng.k, eng.D
        self._work = torch.empty(int(self.lib.ctfit_work_len(self.k, self.D)), dtype=torch.int64, device=self.device)
        self.launch_info = ""

    def update(self, x: torch.Tensor, seq_off, hn_g: float, hn_beta_vec):
        """``x``: the adopted sample; ``seq_off``: S + 1 host int64 with at least one non-empty sequence.  Returns
        ``(n, bad)``; with ``bad > 0`` no table has changed."""
        eng, dev, lib = self.eng, self.device, self.lib
        n, S = int(x.shape[0]), len(seq_off) - 1
        hoff = head_offsets(seq_off, self.D)
        H = int(hoff[-1])
        seq = torch.as_tensor(np.ascontiguousarray(seq_off, dtype=np.int64), device=dev)
        hof = torch.as_tensor(hoff, device=dev)
        hb = torch.as_tensor(np.asarray(hn_beta_vec, dtype=np.float64), device=dev)
        keys = torch.empty(2, H, dtype=torch.int64, device=dev)
        sample = (_CODES[x.dtype], x.data_ptr(), n, seq.data_ptr(), hof.data_ptr(), S, H, self.k, self.D)
        with torch.cuda.device(dev):
            _check(lib.ctfit_count(*sample, eng._out.data_ptr(), keys.data_ptr(), self._work.data_ptr(), stream_ptr(dev)),
                   "ctfit_count")
            got_n, bad = (int(v) for v in eng._out[:2].cpu())
            assert got_n == n
            if bad > 0:
                return n, bad
            ordered = torch.stack([torch.sort(keys[0]).values, torch.sort(keys[1]).values])
            head = torch.empty(int(lib.ctfit_head_len(H)), dtype=torch.int64, device=dev)
            _check(lib.ctfit_rank(*sample, ordered.data_ptr(), eng.beta.data_ptr(), eng.exists.data_ptr(), hb.data_ptr(),
                                  head.data_ptr(), self._work.data_ptr(), stream_ptr(dev)), "ctfit_rank")
            _check(lib.ctfit_sweep(self.k, self.D, eng._out.data_ptr() + 16, eng.beta.data_ptr(), eng.g.data_ptr(),
                                   eng.exists.data_ptr(), float(hn_g), hb.data_ptr(), self._work.data_ptr(), stream_ptr(dev)),
                   "ctfit_sweep")
        oD = eng.off[eng.D]
        eng.leaf[oD:] = eng.exists[oD:]           # a node at the maximal depth is a leaf from its creation on
        self.launch_info = "ctfit_count + sort + ctfit_rank + ctfit_sweep"
        return n, bad
