"""ctypes binding of the Student-t mixture log-density of ``libgmmvb.so`` (C ABI in ``include/stmix.h``).

``StudentMixturePass`` evaluates ``ln p(x_i) = logsumexp_k [c_k - a_k log1p(q_ik / nu_k)]`` (and the first arg-max) for the
rows of a sample in one launch: the predictive read-out behind ``gaussianmixture.LearnModel.calc_pred_logpdf`` and, with one
component, ``multivariate_normal.LearnModel.calc_pred_logpdf`` ("Predictive log-density of a sample").  What is
K-sized - the constants ``c_k`` and the triangular factors - is formed here in float64 torch, on the device of its inputs;
everything N-sized is the library's.  No ``DataPass`` workspace, no [N, K] array, no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import torch

from ._engine import EngineLimitError
from ._native import bind, gpu_device, stream_ptr
from ._regression import _code, adopt_tensor

MAX_DEGREE = 19200                       # include/stmix.h: STMIX_MAX_DEGREE
MAX_COMPONENTS = 65536                   # include/stmix.h: STMIX_MAX_COMPONENTS
LGAMMA_SERIES_FROM = 64.0                # csrc/mvnseq_kernels.h: lgamma_step's threshold

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/stmix.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "stmix_abi_version": (_int, []),
    "stmix_last_error": (ctypes.c_char_p, []),
    "stmix_image_len": (_i64, [_int, _int]),
    "stmix_pack": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp]),
    "stmix_logpdf": (_int, [_int, _int, _int, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("stmix", SYMBOLS)


def image_len(K: int, D: int) -> int:
    """``stmix_image_len`` in Python (csrc/stmix_kernels.h: image_doubles)."""
    if D > 128:
        return K * (D * D + D)
    t = (D + 15) // 16
    return K * ((t * (t + 1) // 2 * 256 + 16 * t + 127) // 128 * 128)


# ---- the K-sized part --------------------------------------------------------------------------------------------------------
def _stirling_tail(x):
    r = 1.0 / x
    r2 = r * r
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))))


def lgamma_step(a: torch.Tensor, h: float) -> torch.Tensor:
    """lnGamma(a + h) - lnGamma(a), h > 0.  From a = 64 on the two lgamma values agree in their leading digits (at a = 5e7
    each is 1e9 and the difference 1e3), so the difference of the two Stirling series is formed instead:
    (a - 1/2) log1p(h / a) + h ln(a + h) - h + t(a + h) - t(a) - what csrc/mvnseq_kernels.h's lgamma_step does on the
    device, restated for K values."""
    big = a >= LGAMMA_SERIES_FROM
    s = torch.where(big, a, torch.full_like(a, LGAMMA_SERIES_FROM))
    series = (s - 0.5) * torch.log1p(h / s) + h * torch.log(s + h) - h + (_stirling_tail(s + h) - _stirling_tail(s))
    return torch.where(big, series, torch.lgamma(a + h) - torch.lgamma(a))


def log_norm_consts(pi: torch.Tensor, nu: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """c_k = ln pi_k + lnGamma((nu_k + D) / 2) - lnGamma(nu_k / 2) - (D / 2) ln(nu_k pi) + sum_j ln U_k[j][j], float64 [K]."""
    D = u.shape[-1]
    h = 0.5 * D
    return (torch.log(pi) + lgamma_step(0.5 * nu, h) - h * torch.log(nu * math.pi)
            + torch.log(torch.diagonal(u, dim1=1, dim2=2)).sum(dim=1))


def precision_factor(cov: torch.Tensor) -> torch.Tensor:
    """Lower triangular U [K, D, D] with U^T U = cov^-1 for a batch of SPD matrices: cov = G G^T, U = G^-1 - the K-side's own
    factorisation (``gmmvb_kside_factor`` on a GPU up to D = 128, ``_kside._factor_checked`` elsewhere); no matrix is
    inverted on the host."""
    from . import _kside
    if cov.is_cuda and cov.shape[-1] <= 128:
        from ._engine import kside_factor
        return kside_factor(cov.contiguous())[1]
    return _kside._factor_checked(cov)[1]


def check_shape(K: int, D: int, who: str):
    if D > MAX_DEGREE or K > MAX_COMPONENTS:
        raise EngineLimitError(f"bayesml_amd.{who} evaluates the predictive log-density for c_degree <= {MAX_DEGREE} and "
                               f"up to {MAX_COMPONENTS} components in this version (got {D}, {K})")


class StudentMixturePass:
    """The log-density pass for mixtures of K Student-t components in D dimensions on one device."""

    def __init__(self, K: int, D: int, device):
        check_shape(K, D, "gaussianmixture")
        self.K, self.D = int(K), int(D)
        self.lib = load_library()
        self.device = gpu_device(device, "Student-t mixture log-density")
        slots = int(self.lib.stmix_image_len(self.K, self.D))
        assert slots == image_len(self.K, self.D)
        self.img = torch.empty(slots, dtype=torch.float64, device=self.device)
        self.launch_info = ""
        self.last = None

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def run(self, x: torch.Tensor, pi, mu, nu, u, want_z: bool, pivot=None):
        """(ln p [n] float64, z [n] int64 or None) as device tensors for the rows x [n, D] (f32 or f64, read where they
        lie) under weights pi [K], locations mu [K, D], degrees of freedom nu [K] and lower triangular u [K, D, D] with
        u^T u the scale (precision) matrices.  ``pivot`` [D] defaults to row 0 of x, read on the device.  Enqueues only."""
        K, D, dev = self.K, self.D, self.device
        n = int(x.shape[0])
        ldx = x.stride(0) if n > 1 else D
        t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()      # noqa: E731
        pi, mu, nu, u = t(pi), t(mu), t(nu), t(u)
        assert pi.shape == (K,) and mu.shape == (K, D) and nu.shape == (K,) and u.shape == (K, D, D)
        pivot = x[0].to(torch.float64).contiguous() if pivot is None else t(pivot)
        c = log_norm_consts(pi, nu, u)
        lnp = torch.empty(n, dtype=torch.float64, device=dev)
        z = torch.empty(n, dtype=torch.int64, device=dev) if want_z else None
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            _check(self.lib.stmix_pack(K, D, u.data_ptr(), mu.data_ptr(), pivot.data_ptr(), self.img.data_ptr(), stream),
                   "stmix_pack")
            _check(self.lib.stmix_logpdf(K, D, _code(x.dtype), x.data_ptr(), ldx, n, pivot.data_ptr(), self.img.data_ptr(),
                                         c.data_ptr(), nu.data_ptr(), lnp.data_ptr(), None if z is None else z.data_ptr(),
                                         stream), "stmix_logpdf")
        # (what the engine was handed: the tests' oracle starts from exactly these)
        self.last = dict(pi=pi, mu=mu, nu=nu, u=u, pivot=pivot, c=c)
        self.launch_info = f"stmix_logpdf ({'plain f64' if D > 128 else 'fused f64 MFMA'}, K={K}, D={D}, {n} rows)"
        return lnp, z

    def close(self):
        pass


# ---- what the two models share --------------------------------------------------------------------------------------------------
def model_logpdf(model, who: str, x, as_numpy: bool, K: int, params, want_z: bool):
    """``calc_pred_logpdf`` of a model: the engine (or the stand-in behind the private seam ``model._stmix_pass_factory``),
    the parameters ``params(device) -> (pi, mu, nu, u)`` on the engine's device, the pass, and the return kinds - NumPy for
    a NumPy sample, tensors on the model's device otherwise."""
    D = model.c_degree
    n = int(x.shape[0])
    if n == 0:
        lnp, z = torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int64)
    else:
        check_shape(K, D, who)
        make = model._stmix_pass_factory
        eng = make(K, D) if make is not None else StudentMixturePass(K, D, model._device)
        xd = eng.adopt(x)
        lnp, z = eng.run(xd, *params(eng.device), want_z)
    if as_numpy:
        lnp = lnp.detach().to("cpu").numpy()
        z = z.detach().to("cpu").numpy() if want_z else None
    return (lnp, z) if want_z else lnp
