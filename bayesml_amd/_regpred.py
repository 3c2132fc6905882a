"""ctypes binding of the regression scoring and many-series passes of ``libgmmvb.so`` (C ABI in ``include/regpred.h``).

``RegressionScorePass`` evaluates the Student-t predictive log-density of held-out rows under a fixed Normal-Gamma posterior
in one fused pass (``regpred_logpdf``; no p_ms / p_lambdas arrays exist), the same over the lag windows of S independent
series laid end to end (``regpred_logpdf_window``), the statistics block of those windows (``regpred_stats_window``) and
per-series sums and the grand total in a fixed order (``regpred_totals``).  The two offset tables of a call are S-sized,
made here with NumPy and uploaded once; nothing n-sized is built.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ._native import bind, gpu_device, stream_ptr
from ._regression import PAD_ZEROS, _code, adopt_tensor, check_features

_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
# every symbol include/regpred.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "regpred_abi_version": (_int, []),
    "regpred_last_error": (ctypes.c_char_p, []),
    "regpred_work_len": (_i64, [_int]),
    "regpred_logpdf": (_int, [_int, _int, _vp, _i64, _int, _vp, _i64, _vp, _vp, _dbl, _dbl, _dbl, _vp, _vp, _vp]),
    "regpred_logpdf_window": (_int, [_int, _int, _vp, _i64, _int, _i64, _vp, _vp, _i64, _vp, _vp, _dbl, _dbl, _dbl, _vp, _vp,
                                     _vp]),
    "regpred_stats_work_len": (_i64, [_int]),
    "regpred_stats_window": (_int, [_int, _int, _vp, _i64, _int, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "regpred_totals_work_len": (_i64, [_i64]),
    "regpred_totals": (_int, [_i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("regpred", SYMBOLS)


def row_offsets(off: np.ndarray, p: int, padding: int) -> np.ndarray:
    """The S + 1 row offsets of the series with value offsets ``off``: with zeros before a series' start every value is a
    row, otherwise the first p values of a series are initial values only (a series of at most p values has no row)."""
    lens = np.diff(off)
    rows = lens if padding == PAD_ZEROS else np.maximum(lens - p, 0)
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def student_consts(alpha: float, beta: float):
    """(scale, nu, c0) of the predictive Student-t: alpha / beta, 2 alpha and its log-normaliser without the ln(lambda) / 2."""
    nu = 2.0 * float(alpha)
    return float(alpha) / float(beta), nu, math.lgamma((nu + 1.0) / 2.0) - math.lgamma(nu / 2.0) - 0.5 * math.log(math.pi * nu)


class RegressionScorePass:
    """The passes of ``include/regpred.h`` for models of D coefficients on one device."""

    def __init__(self, D: int, device):
        check_features(D, "regression")
        self.D = int(D)
        self.lib = load_library()
        self.device = gpu_device(device, "regression data passes")
        self._work = torch.empty(int(self.lib.regpred_work_len(self.D)), dtype=torch.float64, device=self.device)
        self._swork = self._mu_d = self._linv_d = None
        self.launch_info = ""

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def _posterior(self, mu, linv):
        # (kept on the pass: they must outlive the kernels, which only read them on this stream)
        self._mu_d = torch.as_tensor(np.ascontiguousarray(mu, dtype=np.float64)).to(self.device)
        self._linv_d = torch.as_tensor(np.ascontiguousarray(linv, dtype=np.float64)).to(self.device)
        return self._mu_d.data_ptr(), self._linv_d.data_ptr()

    def tables(self, off: np.ndarray, roff: np.ndarray):
        """The two offset tables of a call on the device, in one upload: (off_d, roff_d), [S + 1] int64 each."""
        both = torch.from_numpy(np.stack([off, roff]).astype(np.int64)).to(self.device)
        return both[0], both[1]

    def logpdf(self, x: torch.Tensor, y: torch.Tensor, mu, linv, consts) -> torch.Tensor:
        """ln St(y_n | x_n . mu, scale / (1 + |linv x_n|^2), nu) of the rows x [n, D] with targets y [n], n >= 1."""
        y = y.contiguous()
        n = int(x.shape[0])
        lnp = torch.empty(n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.regpred_logpdf(self.D, _code(x.dtype), x.data_ptr(), x.stride(0) if n > 1 else self.D,
                                           _code(y.dtype), y.data_ptr(), n, *self._posterior(mu, linv), *consts, lnp.data_ptr(),
                                           self._work.data_ptr(), stream_ptr(self.device)), "regpred_logpdf")
        self.launch_info = "regpred_logpdf"
        return lnp

    def logpdf_window(self, series: torch.Tensor, padding: int, off_d, roff_d, n_rows: int, mu, linv, consts) -> torch.Tensor:
        """The same for the n_rows lag windows (degree D - 1) of the series with the tables ``tables(off, roff)``."""
        lnp = torch.empty(n_rows, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.regpred_logpdf_window(self.D - 1, _code(series.dtype), series.data_ptr(), series.shape[0],
                                                  int(padding), off_d.shape[0] - 1, off_d.data_ptr(), roff_d.data_ptr(), n_rows,
                                                  *self._posterior(mu, linv), *consts, lnp.data_ptr(), self._work.data_ptr(),
                                                  stream_ptr(self.device)), "regpred_logpdf_window")
        self.launch_info = "regpred_logpdf_window"
        return lnp

    def stats_window(self, series: torch.Tensor, padding: int, off_d, roff_d, n_rows: int) -> torch.Tensor:
        """[G | c | s | n] (``include/regvb.h``) over the same windows."""
        if self._swork is None:
            self._swork = torch.empty(int(self.lib.regpred_stats_work_len(self.D)), dtype=torch.float64, device=self.device)
        out = torch.empty(self.D * self.D + self.D + 2, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.regpred_stats_window(self.D - 1, _code(series.dtype), series.data_ptr(), series.shape[0],
                                                 int(padding), off_d.shape[0] - 1, off_d.data_ptr(), roff_d.data_ptr(), n_rows,
                                                 out.data_ptr(), self._swork.data_ptr(), stream_ptr(self.device)),
                   "regpred_stats_window")
        self.launch_info = "regpred_stats_window"
        return out

    def totals(self, lnp: torch.Tensor, roff_d=None, grand: bool = False):
        """(tot [S] or None, total [1] or None): the sums of ``lnp`` per series of ``roff_d`` and over all rows."""
        n = int(lnp.shape[0])
        tot = torch.empty(roff_d.shape[0] - 1, dtype=torch.float64, device=self.device) if roff_d is not None else None
        total = work = None
        if grand:
            total = torch.empty(1, dtype=torch.float64, device=self.device)
            work = torch.empty(int(self.lib.regpred_totals_work_len(n)), dtype=torch.float64, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()                      # noqa: E731
        with torch.cuda.device(self.device):
            _check(self.lib.regpred_totals(0 if tot is None else tot.shape[0], ptr(roff_d), n, lnp.data_ptr(), ptr(tot),
                                           ptr(total), ptr(work), stream_ptr(self.device)), "regpred_totals")
        return tot, total

    def close(self):
        self._work = self._swork = self._mu_d = self._linv_d = None
