"""ctypes binding of the scalar conjugate families of ``libgmmvb.so`` (C ABI in ``include/expfam.h``) over PyTorch-ROCm
tensors, and what the five model packages built on it share.

The division of labour is ``_regression``'s: PyTorch owns device memory and the stream; the one pass over the sample that
checks the family's domain and forms every sum is a gfx950 kernel of ``csrc/expfam_kernels.h``; the closed forms on the
handful of numbers it returns are host code in the model packages.  No CPU fallback: without the library or a GPU,
``ExpfamPass`` raises ``EngineUnavailableError``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._engine import EngineError, EngineLimitError
from ._native import PLOT_MSG, bind, gpu_device, stream_ptr  # noqa: F401  (PLOT_MSG: the model packages read it here)

BERNOULLI, COUNTS, ONEHOT, POISSON, EXPONENTIAL, NORMAL = range(6)      # enum expfam_family
U8, I32, I64, F32, F64 = range(5)                                      # enum expfam_dtype
MAX_DEGREE = 4096         # include/expfam.h: EXPFAM_MAX_DEGREE (int64 histogram bins of a workgroup in LDS)

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/expfam.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "expfam_abi_version": (_int, []),
    "expfam_last_error": (ctypes.c_char_p, []),
    "expfam_stats_len": (_i64, [_int, _int]),
    "expfam_work_len": (_i64, [_int, _int]),
    "expfam_stats_bernoulli": (_int, [_int, _vp, _i64, _vp, _vp, _vp]),
    "expfam_stats_counts": (_int, [_int, _vp, _i64, _int, _vp, _vp, _vp]),
    "expfam_stats_onehot": (_int, [_int, _vp, _i64, _int, _i64, _vp, _vp, _vp]),
    "expfam_stats_poisson": (_int, [_int, _vp, _i64, _vp, _vp, _vp]),
    "expfam_stats_exponential": (_int, [_int, _vp, _i64, _vp, _vp, _vp]),
    "expfam_stats_normal": (_int, [_int, _vp, _i64, _vp, _vp, _vp]),
}
_ENTRY = {BERNOULLI: "expfam_stats_bernoulli", COUNTS: "expfam_stats_counts", ONEHOT: "expfam_stats_onehot",
          POISSON: "expfam_stats_poisson", EXPONENTIAL: "expfam_stats_exponential", NORMAL: "expfam_stats_normal"}
_CODES = {torch.uint8: U8, torch.int32: I32, torch.int64: I64, torch.float32: F32, torch.float64: F64}

load_library, _check = bind("expfam", SYMBOLS)


def check_degree(c_degree: int, what: str):
    """Raised at model construction: a workgroup's histogram bins live in LDS and there is no slower path behind them
    (the reference has no such limit)."""
    if c_degree > MAX_DEGREE:
        raise EngineLimitError(f"bayesml_amd.{what} supports at most {MAX_DEGREE} categories in this version "
                               f"(got {c_degree}); bayesml itself has no such limit")


def code(dtype):
    """expfam_dtype of a tensor the kernels can read; anything else must have been widened by adopt_tensor."""
    try:
        return _CODES[dtype]
    except KeyError:
        raise TypeError(f"the expfam kernels read uint8, int32, int64, float32 or float64, not {dtype}") from None


def adopt_tensor(a, device, kind, cols=None):
    """The sample as a tensor on ``device`` in a dtype the kernels read.  ``kind`` is 'i' (integer family) or 'f'.

    A tensor already there is used in place (a view at any element offset; a row matrix may keep its row stride); a NumPy
    array is copied once.  Dtypes the kernels cannot read are widened, never narrowed: other integer dtypes to int64,
    float16 / bfloat16 to float32, and for 'f' an integer sample to float64 (the reference's ``astype(float)``).
    With ``cols`` the result is [rows, cols] (the one-hot form), otherwise 1-dimensional: the sample is a bag of values."""
    if isinstance(a, torch.Tensor):
        t = a.to(device)
    else:
        a = np.asarray(a)
        if a.dtype.kind == "u" and a.dtype.itemsize > 1:          # torch has no arithmetic on the wider unsigned dtypes
            a = a.astype(np.int64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if kind == "i":
        if t.dtype not in (torch.uint8, torch.int32, torch.int64):
            t = t.to(torch.int64)
    elif t.dtype in (torch.float16, torch.bfloat16):
        t = t.to(torch.float32)
    elif t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if cols is None:
        return t.reshape(-1) if t.is_contiguous() else t.contiguous().reshape(-1)
    if t.dim() == 2 and t.shape[1] == cols and t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= cols):
        return t
    return t.contiguous().reshape(-1, cols)


def decode(family, block):
    """A statistics block (int64 tensor or array, layout in include/expfam.h) as a dict of host numbers."""
    b = block.detach().to("cpu").numpy() if isinstance(block, torch.Tensor) else np.asarray(block)
    f = b.view(np.float64)
    if family == BERNOULLI:
        return dict(n=int(b[0]), bad=int(b[1]), n1=int(b[2]), n0=int(b[3]))
    if family == COUNTS:
        return dict(n=int(b[0]), bad=int(b[1]), max=int(b[2]), counts=b[3:].copy())
    if family == ONEHOT:
        return dict(n=int(b[0]), bad=int(b[1]), counts=b[2:].copy())
    if family == POISSON:
        return dict(n=int(b[0]), bad=int(b[1]), sum=b[2], sum_lgamma=f[3])
    if family == EXPONENTIAL:
        return dict(n=int(b[0]), bad=int(b[1]), sum=f[2])
    return dict(n=int(b[0]), mean=f[1], m2=f[2])


class ExpfamPass:
    """The data passes of the six entry points on one device.  The scratch does not depend on the sample's length (1024
    slabs of a few slots; 1024 x (degree + 2) slots for the categorical passes) and is allocated once per (family, degree)."""

    def __init__(self, device=None):
        self.lib = load_library()
        self.device = gpu_device(device, "scalar conjugate data passes")
        self._work = {}
        self.launch_info = ""

    def adopt(self, a, kind, cols=None):
        return adopt_tensor(a, self.device, kind, cols)

    def stats(self, family: int, x: torch.Tensor, degree: int = 0) -> torch.Tensor:
        """The family's statistics block of the adopted sample x, as an int64 tensor on the device (binary64 slots are
        read through ``.view(torch.float64)``; ``decode`` does it on the host)."""
        n_slots = int(self.lib.expfam_stats_len(family, degree))
        if n_slots < 0:
            check_degree(degree, "categorical")
            raise EngineError(f"expfam_stats_len({family}, {degree}): bad family or degree")
        key = (family, degree)
        if key not in self._work:
            self._work[key] = torch.empty(int(self.lib.expfam_work_len(family, degree)), dtype=torch.int64, device=self.device)
        work = self._work[key]
        out = torch.empty(n_slots, dtype=torch.int64, device=self.device)
        fn = getattr(self.lib, _ENTRY[family])
        with torch.cuda.device(self.device):
            stream = stream_ptr(self.device)
            head = (code(x.dtype), x.data_ptr(), x.shape[0])
            if family == COUNTS:
                rc = fn(*head, degree, out.data_ptr(), work.data_ptr(), stream)
            elif family == ONEHOT:
                ld = x.stride(0) if x.shape[0] > 1 else degree
                rc = fn(*head, degree, ld, out.data_ptr(), work.data_ptr(), stream)
            else:
                rc = fn(*head, out.data_ptr(), work.data_ptr(), stream)
        _check(rc, _ENTRY[family])
        self.launch_info = _ENTRY[family]
        return out

    def close(self):
        self._work = {}


class PassOwner:
    """What the five LearnModels share: the keyword-only ``device``, the lazily made ``ExpfamPass`` (dropped on pickling),
    and the private test seam ``_expfam_pass_factory`` (tests/fake_expfam_engine.py).  The sequence pass behind
    ``pred_and_update_sequence`` (``_expseq.SequencePass``) is made on first use, with its own seam
    ``_expseq_pass_factory`` (tests/expfam_seq_oracle.py); both names are class attributes until then, so a model that
    never calls the method keeps the instance ``__dict__`` and the pickles it always had."""

    _seq_engine = None
    _expseq_pass_factory = None

    def _init_pass(self, device):
        self._device = device
        self._engine = None
        self._expfam_pass_factory = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        state.pop("_seq_engine", None)
        return state

    def _seq_pass(self):
        if self._expseq_pass_factory is not None:
            return self._expseq_pass_factory()
        if self._seq_engine is None:
            from ._expseq import SequencePass
            self._seq_engine = SequencePass(self._device)
        return self._seq_engine

    def _pass(self):
        if self._expfam_pass_factory is not None:
            return self._expfam_pass_factory()
        if self._engine is None:
            self._engine = ExpfamPass(self._device)
        return self._engine

    def _sample_stats(self, family, x, kind, degree=0, cols=None):
        """One pass over an array sample: the decoded statistics block."""
        eng = self._pass()
        return decode(family, eng.stats(family, eng.adopt(x, kind, cols), degree))


def is_array(x):
    return type(x) is np.ndarray or isinstance(x, torch.Tensor)


def size_of(x):
    return int(x.numel()) if isinstance(x, torch.Tensor) else int(x.size)

