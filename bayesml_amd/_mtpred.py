"""ctypes binding of the meta-tree predictive log-density of ``libgmmvb.so`` (C ABI in ``include/mtpred.h``).

``LogpdfPass`` borrows the forest struct and the tables ``post``, ``g``, ``prob`` of a ``_mtree.MtreePass`` and scores
labelled rows under them in one device pass (``csrc/mtpred_kernels.h``): per-node constants once per call, then a tile of 64
rows per workgroup, its features staged in LDS and reused by every tree, the fold and the mixture of the trees in the log
domain.  Nothing is learnt and no table of the engine is written.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch

from ._mtree import _CODES, _fp, _ptr, F64, LINREG, U8
from ._native import bind, stream_ptr

TILE, WAVES, LDS_BYTES, SHARE, LR_CONSTS = 64, 4, 32768, 16, 260          # include/mtpred.h

_vp, _i64, _i32, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int
# every symbol include/mtpred.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mtpred_abi_version": (_int, []),
    "mtpred_last_error": (ctypes.c_char_p, []),
    "mtpred_consts_len": (_i64, [_i32, _int, _int]),
    "mtpred_work_len": (_i64, [_i64, _int]),
    "mtpred_logpdf": (_int, [_fp, _int, _int, _int, _vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("mtpred", SYMBOLS)


def staged(dim_cont: int, dim_cat: int) -> bool:
    """Whether a tile's features fit the LDS budget (``mtpred_logpdf`` decides the same way)."""
    return TILE * (8 * dim_cont + 4 * dim_cat) <= LDS_BYTES


class LogpdfPass:
    """``mtpred_logpdf`` on the forest and the posterior tables of the engine ``eng``."""

    def __init__(self, eng):
        self.lib = load_library()
        self.eng, self.device = eng, eng.device
        need = int(self.lib.mtpred_consts_len(eng.flat.n_nodes, eng.family, eng.degree))
        assert need > 0
        self._consts = torch.empty(need, dtype=torch.float64, device=self.device)
        self.launch_info = ""

    def run(self, xc, xk, y, total=False):
        """``xc``, ``xk``, ``y``: the engine's adopted rows and labels.  Returns ``(lnp[n], total or None)`` on the device
        (enqueue only)."""
        eng = self.eng
        n = int(y.shape[0])
        lnp = torch.empty(n, dtype=torch.float64, device=self.device)
        tot = torch.empty(1, dtype=torch.float64, device=self.device) if total else None
        work = torch.empty(int(self.lib.mtpred_work_len(n, 1)), dtype=torch.float64, device=self.device) if total else None
        cc, ck = (_CODES[xc.dtype] if xc is not None else F64), (_CODES[xk.dtype] if xk is not None else U8)
        with torch.cuda.device(self.device):
            rc = self.lib.mtpred_logpdf(ctypes.byref(eng.struct), eng.family, eng.degree, cc, _ptr(xc), ck, _ptr(xk),
                                        y.data_ptr(), n, eng.post.data_ptr(), eng.g.data_ptr(), eng.prob.data_ptr(),
                                        self._consts.data_ptr(), lnp.data_ptr(), _ptr(tot), _ptr(work),
                                        stream_ptr(self.device))
        _check(rc, "mtpred_logpdf")
        form = "staged" if staged(eng.dim_cont, eng.dim_cat) else "direct"
        self.launch_info = (f"mtpred_logpdf ({form}" + (", matrix pipe from %d lanes" % SHARE if eng.family == LINREG else "")
                            + ")" + (" + total" if total else ""))
        return lnp, tot
