"""ctypes binding of the scalar conjugate families' prequential pass of ``libgmmvb.so`` (C ABI in ``include/expseq.h``),
and the ``pred_and_update_sequence`` that the model packages built on ``_expfam`` share.

The division of labour is ``_expfam``'s: PyTorch owns device memory and the stream; the exclusive prefix scan of the
sufficient statistics over the sample, the predictive parameters of every position and the code lengths are gfx950 kernels
of ``csrc/expseq_kernels.h``; the predictions are vectorised copies of each class's ``make_prediction`` on the parameter
arrays the pass returns, NumPy for a NumPy sample and torch on the device for a tensor.  No CPU fallback: without the
library or a GPU, ``SequencePass`` raises ``EngineUnavailableError``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _expfam as xf
from ._engine import EngineError
from ._exceptions import CriteriaError
from ._native import bind, gpu_device, stream_ptr

BERNOULLI, POISSON, EXPONENTIAL, NORMAL, CATEGORICAL = range(5)          # enum expseq_family
# the fixed tree of csrc/expseq_kernels.h (tests/expfam_seq_oracle.py adds in this order)
TILE = 2048               # include/expseq.h: EXPSEQ_TILE, positions of a workgroup
SCAN_THREADS = 256        # include/expseq.h: EXPSEQ_SCAN_THREADS, threads of the one workgroup that scans the tiles
THREADS = 256             # threads of a tile's workgroup (waves of 64)
ITEMS = TILE // THREADS   # consecutive positions of a thread
SLOTS = 4                 # 8-byte slots of a tile's aggregate and of its carry
CHUNK_BYTES = 256 << 20   # default bound of the categorical pass's scratch, the one that grows with n and c_degree

PARAMS = {BERNOULLI: ("p_theta",), POISSON: ("p_r", "p_theta"), EXPONENTIAL: ("p_kappa", "p_lambda"),
          NORMAL: ("p_mu", "p_nu", "p_lambda")}
KIND = {BERNOULLI: "i", POISSON: "i", EXPONENTIAL: "f", NORMAL: "f"}
N_START = {BERNOULLI: 2, POISSON: 2, EXPONENTIAL: 2, NORMAL: 4}

_vp, _i64, _int, _dp = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
# every symbol include/expseq.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "expseq_abi_version": (_int, []),
    "expseq_last_error": (ctypes.c_char_p, []),
    "expseq_work_len": (_i64, [_int, _int, _i64]),
    "expseq_bernoulli": (_int, [_int, _vp, _i64, _dp, _vp, _vp, _vp, _vp, _vp]),
    "expseq_poisson": (_int, [_int, _vp, _i64, _dp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "expseq_exponential": (_int, [_int, _vp, _i64, _dp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "expseq_normal": (_int, [_int, _vp, _i64, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "expseq_categorical": (_int, [_int, _vp, _i64, _int, _int, _i64, _vp, ctypes.c_double, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
_ENTRY = {BERNOULLI: "expseq_bernoulli", POISSON: "expseq_poisson", EXPONENTIAL: "expseq_exponential", NORMAL: "expseq_normal"}

load_library, _check = bind("expseq", SYMBOLS)


def work_len(family: int, degree: int, m: int) -> int:
    """``expseq_work_len`` restated: an aggregate and a carry of SLOTS slots per tile of the m positions; for the
    categorical pass a histogram and a bad count per tile and m row indices."""
    tiles = (m + TILE - 1) // TILE
    if family == CATEGORICAL:
        return tiles * (degree + 1) + m if 1 <= degree <= xf.MAX_DEGREE and m >= 1 else -1
    if family not in PARAMS or degree != 0 or m < 1:
        return -1
    return 2 * SLOTS * tiles


def chunk_len(degree: int, chunk_bytes=None) -> int:
    """Positions of one categorical chunk: the largest m whose scratch, ``8 * work_len(CATEGORICAL, degree, m)`` bytes,
    stays within ``chunk_bytes``; at least one."""
    budget = int(CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
    per_tile = 8 * (degree + 1 + TILE)
    full = budget // per_tile
    return max(1, full * TILE + max(0, (budget - full * per_tile - 8 * (degree + 1)) // 8))


class SequencePass:
    """The prequential passes of include/expseq.h on one device.  The scratch is 8 slots per tile of the sample; the
    categorical pass's is c_degree + 1 slots per tile of a chunk and one slot per position of it (the row indices of the
    one-hot form)."""

    def __init__(self, device=None):
        self.lib = load_library()
        self.device = gpu_device(device, "scalar conjugate sequence passes")
        self.launch_info = ""

    def adopt(self, a, kind, cols=None):
        return xf.adopt_tensor(a, self.device, kind, cols)

    def run(self, family: int, x: torch.Tensor, start, params: bool = True, nats: bool = True):
        """One pass over the adopted sample x (n >= 1) from the start posterior ``start`` (the slots of include/expseq.h).
        Returns ``(parameter arrays, nats, status)``: a tuple of float64 [n] device tensors in the order of
        ``PARAMS[family]`` (None without ``params``), the code lengths (None without ``nats``), and the int64 [1] count of
        values outside the family's domain.  Nothing is synchronised."""
        n = int(x.shape[0])
        start = [float(v) for v in start]
        if len(start) != N_START[family]:
            raise EngineError(f"{_ENTRY[family]}: start has {N_START[family]} slots, got {len(start)}")
        wl = int(self.lib.expseq_work_len(family, 0, max(n, 1)))
        new = lambda: torch.empty(n, dtype=torch.float64, device=self.device)          # noqa: E731
        outs = tuple(new() for _ in PARAMS[family]) if params else None
        code = new() if nats else None
        status = torch.empty(1, dtype=torch.int64, device=self.device)
        work = torch.empty(max(wl, 1), dtype=torch.int64, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        c_start = (ctypes.c_double * len(start))(*start)
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, _ENTRY[family])(
                xf.code(x.dtype), x.data_ptr(), n, c_start, *[ptr(t) for t in (outs or (None,) * len(PARAMS[family]))],
                ptr(code), status.data_ptr(), work.data_ptr(), stream_ptr(self.device))
        _check(rc, _ENTRY[family])
        self.launch_info = f"{_ENTRY[family]} (n = {n}, tiles = {(n + TILE - 1) // TILE})"
        return outs, code, status

    def run_categorical(self, x: torch.Tensor, onehot: bool, alpha, want=None, nats: bool = True, chunk_bytes=None):
        """The categorical pass over the adopted sample x ([n] indices, or [n, c_degree] one-hot rows with ``onehot``)
        from the start ``alpha`` = hn_alpha_vec, in chunks of ``chunk_len`` positions with the int64 counts carried on the
        device between them.  ``want`` is None, "rows" (float64 [n, c_degree]) or "argmax" (int64 [n], no row is stored).
        Returns ``(rows or argmax or None, nats or None, counts, status)``; ``self.passes`` counts the chunks."""
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        degree, n = int(alpha.shape[0]), int(x.shape[0])
        m = min(chunk_len(degree, chunk_bytes), n)
        dev = self.device
        alpha_dev = torch.from_numpy(alpha).to(dev)
        s0 = float(alpha.sum())
        counts = torch.zeros(degree, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        work = torch.empty(int(self.lib.expseq_work_len(CATEGORICAL, degree, m)), dtype=torch.int64, device=dev)
        code = torch.empty(n, dtype=torch.float64, device=dev) if nats else None
        rows = torch.empty((n, degree), dtype=torch.float64, device=dev) if want == "rows" else None
        am = torch.empty(n, dtype=torch.int64, device=dev) if want == "argmax" else None
        ld = int(x.stride(0)) if onehot and n > 1 else degree
        part = lambda t, i0: None if t is None else t[i0:].data_ptr()          # noqa: E731
        self.passes = 0
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            for i0 in range(0, n, m):
                rc = self.lib.expseq_categorical(xf.code(x.dtype), x[i0:].data_ptr(), min(m, n - i0), degree, int(bool(onehot)), ld,
                                                 alpha_dev.data_ptr(), s0, i0, counts.data_ptr(), part(code, i0), part(rows, i0),
                                                 part(am, i0), status.data_ptr(), work.data_ptr(), stream)
                _check(rc, "expseq_categorical")
                self.passes += 1
        self.launch_info = f"expseq_categorical x {self.passes} (m = {m}, c_degree = {degree})"
        return (rows if want == "rows" else am), code, counts, status

    def close(self):
        pass


def check_sequence_loss(loss, code_length, losses, loss_msg):
    """``loss`` is one of the class's own losses, or None with ``code_length`` (the wording of ``_normalgamma``)."""
    if loss is None:
        if not code_length:
            raise CriteriaError("loss=None returns the code lengths alone: pass code_length=True with it.")
    elif not (isinstance(loss, str) and loss in losses):
        raise CriteriaError(loss_msg)


def out_device(obj, x):
    """Where the empty results of an empty tensor sample go: the device the pass would have written to (the model's GPU,
    or a stand-in's device).  Without any engine, an empty sample needing none, the sample's own device."""
    if obj._expseq_pass_factory is not None:
        return obj._expseq_pass_factory().device
    if torch.cuda.is_available():
        return gpu_device(obj._device, "scalar conjugate sequence passes")
    return x.device


def host(t):
    """A parameter array as float64 / int64 NumPy (SciPy's distributions are host code)."""
    return t.detach().to("cpu").numpy() if isinstance(t, torch.Tensor) else t


def as_int64(a):
    return a.to(torch.int64) if isinstance(a, torch.Tensor) else a.astype(np.int64)


def xp_of(a):
    """The module whose ``where`` / ``floor`` / ``stack`` / ``zeros_like`` take ``a``."""
    return torch if isinstance(a, torch.Tensor) else np


def sequence(obj, family, x, loss, code_length, losses, loss_msg, accept, fold, start, predict):
    """What the models' ``pred_and_update_sequence`` share.

    1. ``accept()`` is the model's own validated statistics pass over x: it raises what ``update_posterior(x)`` raises,
       with nothing changed yet.
    2. The sequence pass runs from ``start`` (the hn_* slots of include/expseq.h).
    3. ``fold(statistics)`` is ``update_posterior``'s own fold, so hn_* and the bookkeeping are its bits.

    ``predict(loss, params)`` is the vectorised ``make_prediction`` on the tuple of parameter arrays.  A scalar is a
    sample of one; an empty array predicts and learns nothing."""
    check_sequence_loss(loss, code_length, losses, loss_msg)
    stats = accept()
    as_numpy = not isinstance(x, torch.Tensor)
    n = xf.size_of(x) if xf.is_array(x) else 1
    want_params = loss is not None
    if n == 0:
        zero = (lambda: np.zeros(0)) if as_numpy else (lambda: torch.zeros(0, dtype=torch.float64, device=out_device(obj, x)))
        params, nats = tuple(zero() for _ in PARAMS[family]), zero()
    else:
        eng = obj._seq_pass()
        if not xf.is_array(x):
            x = np.asarray([x], dtype=np.int64 if KIND[family] == "i" else np.float64)
        params, nats, _ = eng.run(family, eng.adopt(x, KIND[family]), start, params=want_params, nats=bool(code_length))
        fold(stats)
        if as_numpy:
            params = None if params is None else tuple(host(p) for p in params)
            nats = None if nats is None else host(nats)
    if not want_params:
        return nats
    if n > 0:
        for name, p in zip(PARAMS[family], params):
            setattr(obj, name, float(p[-1]))
    pred = predict(loss, params)
    return (pred, nats) if code_length else pred
