"""ctypes binding of the regression family of ``libgmmvb.so`` (C ABI in ``include/regvb.h``) over PyTorch-ROCm tensors.

The same division of labour as ``_engine``: PyTorch owns device memory and the stream, every N-sized sum is done by the
gfx950 kernels of ``csrc/regvb_kernels.h``.  No CPU fallback: without the library or a GPU, ``RegressionPass`` raises
``EngineUnavailableError``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._engine import EngineLimitError
from ._native import bind, gpu_device, stream_ptr

REGVB_F32, REGVB_F64 = 0, 1
PAD_NONE, PAD_ZEROS = 0, 1
MAX_FEATURES = 256        # include/regvb.h: REGVB_MAX_DEGREE (the f64 MFMA kernels' sixteen feature tiles)

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/regvb.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "regvb_abi_version": (_int, []),
    "regvb_last_error": (ctypes.c_char_p, []),
    "regvb_stats_len": (_i64, [_int]),
    "regvb_stats_work_len": (_i64, [_int]),
    "regvb_stats": (_int, [_int, _int, _vp, _i64, _int, _vp, _i64, _vp, _vp, _vp]),
    "regvb_stats_window": (_int, [_int, _int, _vp, _i64, _int, _vp, _vp, _vp]),
    "regvb_predict_work_len": (_i64, [_int]),
    "regvb_predict": (_int, [_int, _int, _vp, _i64, _i64, _vp, _vp, ctypes.c_double, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("regvb", SYMBOLS)


def check_features(n_features: int, what: str):
    """Raised at model construction: the regression kernels are MFMA kernels for up to 256 features and there is no
    slower path behind them (the reference has no such limit)."""
    if n_features > MAX_FEATURES:
        raise EngineLimitError(f"bayesml_amd.{what} supports at most {MAX_FEATURES} regression coefficients in this "
                               f"version (got {n_features}); bayesml itself has no such limit")


def _code(dtype):
    """regvb_dtype of a tensor the kernels can read; anything else must have been widened by adopt_tensor."""
    if dtype == torch.float32:
        return REGVB_F32
    if dtype == torch.float64:
        return REGVB_F64
    raise TypeError(f"the regression kernels read float32 or float64, not {dtype}")


def adopt_tensor(a, device):
    """Rows [N, D], targets [N] or a series [T] as an f32 / f64 tensor on ``device``, each in its OWN dtype (the kernels
    widen on load; nothing is ever narrowed to match another argument).  A tensor already there is used in place (a row
    matrix may keep its row stride); anything else is copied once; other dtypes are widened to f64."""
    if isinstance(a, torch.Tensor):
        t = a.to(device)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)))
        t = t.to(device)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


class RegressionPass:
    """The three data passes for models of D coefficients on one device.  The scratch does not depend on the number of
    rows (10 to 71 MB, include/regvb.h: regvb_stats_work_len) and is allocated once."""

    def __init__(self, D: int, device):
        check_features(D, "regression")
        self.D = int(D)
        self.lib = load_library()
        self.device = gpu_device(device, "regression data passes")
        self.stats_len = int(self.lib.regvb_stats_len(self.D))
        self._work = torch.empty(int(self.lib.regvb_stats_work_len(self.D)), dtype=torch.float64, device=self.device)
        self._pwork = self._mu_d = self._linv_d = None
        self.launch_info = ""

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def stats(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """[G | c | s | n] of the rows x [N, D] and targets y [N].  x and y keep their own dtypes (f32 or f64): the kernel
        widens each value on load, nothing is narrowed."""
        y = y.contiguous()
        out = torch.empty(self.stats_len, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.regvb_stats(self.D, _code(x.dtype), x.data_ptr(), x.stride(0) if x.shape[0] > 1 else self.D,
                                        _code(y.dtype), y.data_ptr(), x.shape[0], out.data_ptr(), self._work.data_ptr(),
                                        stream_ptr(self.device)), "regvb_stats")
        self.launch_info = "regvb_stats"
        return out

    def stats_window(self, series: torch.Tensor, padding: int) -> torch.Tensor:
        """The same for the lag windows of a series (degree D - 1)."""
        out = torch.empty(self.stats_len, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.regvb_stats_window(self.D - 1, _code(series.dtype), series.data_ptr(), series.shape[0], int(padding),
                                               out.data_ptr(), self._work.data_ptr(), stream_ptr(self.device)),
                   "regvb_stats_window")
        self.launch_info = "regvb_stats_window"
        return out

    def predict(self, x: torch.Tensor, mu, linv, scale: float):
        """(p_ms [N], p_lambdas [N]) on the device: x . mu and scale / (1 + |linv x|^2) per row."""
        if self._pwork is None:
            self._pwork = torch.empty(int(self.lib.regvb_predict_work_len(self.D)), dtype=torch.float64, device=self.device)
        # (kept on the pass: they must outlive the kernels, which only read them on this stream)
        self._mu_d = mu_d = torch.as_tensor(np.ascontiguousarray(mu, dtype=np.float64)).to(self.device)
        self._linv_d = linv_d = torch.as_tensor(np.ascontiguousarray(linv, dtype=np.float64)).to(self.device)
        n = x.shape[0]
        p_ms = torch.empty(n, dtype=torch.float64, device=self.device)
        p_lambdas = torch.empty(n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.regvb_predict(self.D, _code(x.dtype), x.data_ptr(), x.stride(0) if n > 1 else self.D, n,
                                          mu_d.data_ptr(), linv_d.data_ptr(), float(scale), p_ms.data_ptr(),
                                          p_lambdas.data_ptr(), self._pwork.data_ptr(), stream_ptr(self.device)),
                   "regvb_predict")
        self.launch_info = "regvb_predict"
        return p_ms, p_lambdas

    def close(self):
        self._work = self._pwork = self._mu_d = self._linv_d = None
