"""ctypes binding of the HMM sequence predictive of ``libgmmvb.so`` (C ABI in ``include/hmmpred.h``).

``HmmFilterPass`` evaluates ``ln p(x_t | x_0 .. x_{t-1})`` of the rows of a sequence under an HMM with Student-t
emissions, the filtered arg-max path and the last filtered state posterior in one device pass: the read-out behind
``hiddenmarkovnormal.LearnModel.calc_pred_logpdf`` ("Predictive log-density of a sequence").  What is K-sized -
the constants ``c_k`` - is formed here in float64 torch (``_stmix.log_norm_consts`` with pi = 1), the parameter image is
``stmix_pack``'s; everything T-sized is the library's.  No ``DataPass`` workspace, no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _stmix
from ._engine import EngineLimitError
from ._exceptions import ParameterFormatError
from ._native import bind, gpu_device, stream_ptr
from ._regression import _code, adopt_tensor

MAX_DEGREE = 19200                       # include/hmmpred.h: HMMPRED_MAX_DEGREE
MAX_STATES = 256                         # include/hmmpred.h: HMMPRED_MAX_STATES
PARALLEL_STATES = 64                     # include/hmmpred.h: HMMPRED_PARALLEL_STATES
MIN_CHUNK = 8                            # include/hmmpred.h: HMMPRED_MIN_CHUNK
FORGET_TOL = 2e-13                       # csrc/hmmpred.hip: kForgetTol
DEFAULT_CHUNK_BYTES = 1 << 30            # scratch of one time slice of calc_pred_logpdf

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/hmmpred.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "hmmpred_abi_version": (_int, []),
    "hmmpred_last_error": (ctypes.c_char_p, []),
    "hmmpred_scratch_len": (_i64, [_int, _int, _i64]),
    "hmmpred_logpdf": (_int, [_int, _int, _int, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp,
                              _vp, _vp]),
}

load_library, _check = bind("hmmpred", SYMBOLS)


def scratch_len(K: int, D: int, n_rows: int) -> int:
    """``hmmpred_scratch_len`` in Python (csrc/hmmpred.hip: layout): rho' and phi [npad][Kp], s and m [npad], two sets of
    boundary vectors for chunks of MIN_CHUNK steps, the gate."""
    kp = 16 * ((K + 15) // 16)
    npad = (n_rows + 63) // 64 * 64
    chunk_cap = (n_rows - 1 + MIN_CHUNK - 1) // MIN_CHUNK + 1
    return 2 * npad * kp + 2 * npad + 2 * chunk_cap * kp + 2


def default_plan(T: int) -> tuple:
    """(chunk_len, sweep_len) a call with 0, 0 takes (csrc/hmmpred.hip); chunk_len 0 = one serial walk."""
    L = 0 if T < 4096 else (256 if T > 32768 else 32)
    return L, (min(64, L) if L else 0)


def check_shape(K: int, D: int):
    if D > MAX_DEGREE or K > MAX_STATES:
        raise EngineLimitError(f"bayesml_amd.hiddenmarkovnormal evaluates the predictive log-density of a sequence for "
                               f"c_degree <= {MAX_DEGREE} and c_num_classes <= {MAX_STATES} in this version (got {D}, {K})")


class HmmFilterPass:
    """The filter pass for HMMs of K states with Student-t emissions in D dimensions on one device."""

    def __init__(self, K: int, D: int, device):
        check_shape(K, D)
        self.K, self.D = int(K), int(D)
        _stmix.load_library()                # (stmix_pack's prototype: the parameter image is its)
        self.lib = load_library()
        self.device = gpu_device(device, "HMM sequence predictive")
        self.img = torch.empty(int(self.lib.stmix_image_len(self.K, self.D)), dtype=torch.float64, device=self.device)
        self.launch_info = ""
        self.last = None

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def run(self, x: torch.Tensor, a, w0, mu, nu, u, want_z: bool, pivot=None, chunk_len: int = 0, sweep_len: int = 0,
            out=None):
        """(ln p [T] float64, z [T] int64 or None, phi_{T-1} [K], diag [2] int64) as device tensors for the rows x [T, D]
        (f32 or f64, read where they lie) under the transition matrix a [K, K], the first row's state distribution w0 [K],
        locations mu [K, D], degrees of freedom nu [K] and lower triangular u [K, D, D] with u^T u the scale (precision)
        matrices.  ``pivot`` [D] defaults to row 0 of x.  diag: chunks whose start vector did not stand, chunks walked
        again.  ``out``: a dict of caller-made result tensors lnp, z, end, diag to write into.  Enqueues only."""
        K, D, dev = self.K, self.D, self.device
        n = int(x.shape[0])
        ldx = x.stride(0) if n > 1 else D
        t = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()      # noqa: E731
        a, w0, mu, nu, u = t(a), t(w0), t(mu), t(nu), t(u)
        assert a.shape == (K, K) and w0.shape == (K,) and mu.shape == (K, D) and nu.shape == (K,) and u.shape == (K, D, D)
        pivot = x[0].to(torch.float64).contiguous() if pivot is None else t(pivot)
        c = _stmix.log_norm_consts(torch.ones_like(nu), nu, u)
        need = int(self.lib.hmmpred_scratch_len(K, D, n))
        assert need == scratch_len(K, D, n)
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
        if out is not None:
            lnp, z, end, diag = out["lnp"], (out["z"] if want_z else None), out["end"], out["diag"]
            assert lnp.shape == (n,) and end.shape == (K,) and diag.shape == (2,) and (z is None or z.shape == (n,))
            assert all(v is None or (v.is_contiguous() and v.device == dev) for v in (lnp, z, end, diag))
        else:
            lnp = torch.empty(n, dtype=torch.float64, device=dev)
            z = torch.empty(n, dtype=torch.int64, device=dev) if want_z else None
            end = torch.empty(K, dtype=torch.float64, device=dev)
            diag = torch.empty(2, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            _stmix._check(self.lib.stmix_pack(K, D, u.data_ptr(), mu.data_ptr(), pivot.data_ptr(), self.img.data_ptr(), stream),
                          "stmix_pack")
            _check(self.lib.hmmpred_logpdf(K, D, _code(x.dtype), x.data_ptr(), ldx, n, pivot.data_ptr(), self.img.data_ptr(),
                                           c.data_ptr(), nu.data_ptr(), a.data_ptr(), w0.data_ptr(), int(chunk_len),
                                           int(sweep_len), scratch.data_ptr(), lnp.data_ptr(),
                                           None if z is None else z.data_ptr(), end.data_ptr(), diag.data_ptr(), stream),
                   "hmmpred_logpdf")
        # (what the engine was handed: the tests' oracle starts from exactly these)
        self.last = dict(a=a, w0=w0, mu=mu, nu=nu, u=u, pivot=pivot, c=c, chunk_len=int(chunk_len), sweep_len=int(sweep_len),
                         diag=diag)
        self.launch_info = (f"hmmpred_logpdf ({'plain f64' if D > 128 else 'f64 MFMA'} emission, "
                            f"{'chunk-parallel' if K <= PARALLEL_STATES else 'serial'} filter, K={K}, D={D}, {n} rows)")
        return lnp, z, end, diag

    def close(self):
        pass


# ---- the model's method ---------------------------------------------------------------------------------------------------------
def start_vector(model, start) -> np.ndarray:
    """w0 of ``calc_pred_logpdf``: "last", "initial" or a length-K distribution."""
    K = model.c_num_classes
    if isinstance(start, str):
        if start == "last":
            return model._gamma_last @ model.p_a_mat
        if start == "initial":
            return model.hn_eta_vec / model.hn_eta_vec.sum()
        raise ParameterFormatError(f'start="{start}" is unsupported: "last", "initial" or a vector of c_num_classes weights')
    if isinstance(start, torch.Tensor):
        start = start.detach().to("cpu", torch.float64).numpy()
    try:
        w0 = np.array(start, dtype=np.float64)
    except (TypeError, ValueError):
        raise ParameterFormatError('start must be "last", "initial" or a vector of c_num_classes weights') from None
    if w0.shape != (K,) or not np.all(np.isfinite(w0)) or np.any(w0 < 0.0) or abs(w0.sum() - 1.0) > 1e-12:
        raise ParameterFormatError(f"start must have c_num_classes = {K} non-negative entries that sum to 1 within 1e-12")
    return w0


def slice_rows(K: int, D: int, chunk_bytes: int) -> int:
    """The most rows whose scratch fits ``chunk_bytes`` (at least one)."""
    budget = max(0, int(chunk_bytes)) // 8
    lo, hi = 1, 2
    while scratch_len(K, D, hi) <= budget:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:                   # scratch_len(lo) fits (or lo = 1), scratch_len(hi) does not
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if scratch_len(K, D, mid) <= budget else (lo, mid)
    return lo


def model_logpdf(model, x, as_numpy: bool, start, want_z: bool, want_state: bool, chunk_bytes, params):
    """``calc_pred_logpdf`` of the HMM: the start vector, the engine (or the stand-in behind the private seam
    ``model._hmmpred_pass_factory``), the parameters ``params(device) -> (a, mu, nu, u)``, the time slices - each from the
    true phi A of the slice before - and the return kinds."""
    K, D = model.c_num_classes, model.c_degree
    w0 = start_vector(model, start)
    if chunk_bytes is None:
        chunk_bytes = DEFAULT_CHUNK_BYTES
    if not (isinstance(chunk_bytes, (int, np.integer)) and chunk_bytes > 0):
        raise ParameterFormatError("chunk_bytes must be a positive integer")
    n = int(x.shape[0])
    if n == 0:
        lnp, z, state = torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int64), torch.from_numpy(w0.copy())
    else:
        check_shape(K, D)
        make = model._hmmpred_pass_factory
        eng = make(K, D) if make is not None else HmmFilterPass(K, D, model._device)
        xd = eng.adopt(x)
        a, mu, nu, u = params(eng.device)
        w = torch.as_tensor(w0, dtype=torch.float64, device=eng.device)
        step = slice_rows(K, D, chunk_bytes)
        pivot = xd[0].to(torch.float64).contiguous()
        parts, zparts, state = [], [], None
        for lo in range(0, n, step):
            lnp, z, state, _ = eng.run(xd[lo:lo + step], a, w, mu, nu, u, want_z, pivot=pivot)
            parts.append(lnp)
            zparts.append(z)
            w = state @ a
        lnp = parts[0] if len(parts) == 1 else torch.cat(parts)
        z = None if not want_z else (zparts[0] if len(zparts) == 1 else torch.cat(zparts))
    out = [lnp] + ([z] if want_z else []) + ([state] if want_state else [])
    if as_numpy:
        out = [v.detach().to("cpu").numpy() for v in out]
    return out[0] if len(out) == 1 else tuple(out)
