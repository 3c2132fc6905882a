"""ctypes binding of the sequential multivariate-normal engine of ``libgmmvb.so`` (C ABI in ``include/mvnseq.h``).

``MvnSeqPass`` runs ``mvnseq_pass`` over a sample pass by pass: every row's multivariate Student-t predictive from the
posterior of the rows before it, as n calls of ``LearnModel.pred_and_update`` would give it, in eight launches per pass.
The block schedule belongs to the call (it is ``_regseq``'s); a pass is a range of whole blocks of it, sized by the
workspace budget, and passes carry state only through the ``carry`` block, so the cut changes the workspace and nothing
about the arithmetic.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._engine import EngineLimitError
from ._native import bind, gpu_device, stream_ptr
from ._regression import _code, adopt_tensor
from ._regseq import BLOCK, DEFAULT_CHUNK_BYTES, MAX_BLOCKS, block_count, block_start  # noqa: F401  (one schedule)

MAX_DEGREE = 256                         # include/mvnseq.h: MVNSEQ_MAX_DEGREE
OUTPUTS = ("means", "logdet", "quad", "nats")

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/mvnseq.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mvnseq_abi_version": (_int, []),
    "mvnseq_last_error": (ctypes.c_char_p, []),
    "mvnseq_block": (_int, [_int]),
    "mvnseq_block_count": (_i64, [_i64]),
    "mvnseq_block_start": (_i64, [_i64, _i64]),
    "mvnseq_work_len": (_i64, [_int, _i64]),
    "mvnseq_pass": (_int, [_int, _int, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("mvnseq", SYMBOLS)


# ---- the workspace in Python (csrc/mvnseq.hip: layout_of) -------------------------------------------------------------------
def work_slots(D: int, blocks: int) -> int:
    """``mvnseq_work_len`` in Python, so that passes can be planned without the library."""
    tiles = 2 * ((D + 31) // 32)
    slab = tiles * (tiles + 1) // 2 * 256 + 16 * tiles + 16          # regvb_kernels.h: gram_slab_len
    pd = (D + 15) // 16 * 16
    return blocks + 1 + blocks * (pd + BLOCK + BLOCK * D + slab + pd * pd + pd + 2)


def plan_blocks(n: int, D: int, chunk_bytes=None) -> int:
    """Blocks per pass: the largest count whose workspace fits ``chunk_bytes`` (1 if none does), at most the schedule's."""
    budget = DEFAULT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    per_block = work_slots(D, 2) - work_slots(D, 1)
    fit = (budget // 8 - 1) // per_block
    return int(max(1, min(fit, block_count(n), MAX_BLOCKS)))


def start_state(s0, m0, kappa0, nu0):
    """[S_0 = hn_w_mat_inv | m_0 | kappa_0, nu_0] as the passes read it."""
    return np.concatenate([np.asarray(s0, dtype=np.float64).reshape(-1), np.asarray(m0, dtype=np.float64),
                           [float(kappa0), float(nu0)]])


def check_degree(D: int):
    if D > MAX_DEGREE:
        raise EngineLimitError(f"bayesml_amd.multivariate_normal predicts a sequence for c_degree <= {MAX_DEGREE} in this "
                               f"version (got {D}); bayesml itself has no such limit")


class MvnSeqPass:
    """The sequential passes for models of D dimensions on one device."""

    def __init__(self, D: int, device):
        check_degree(D)
        self.D = int(D)
        self.lib = load_library()
        self.device = gpu_device(device, "multivariate-normal sequence passes")
        assert int(self.lib.mvnseq_block(self.D)) == BLOCK
        self.launch_info = ""
        self.passes = 0

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def run(self, x: torch.Tensor, start, want, chunk_bytes=None):
        """The outputs named in ``want`` (of ``OUTPUTS``) as device tensors, a dict: ``means`` [n, D], the others [n],
        for the rows x [n, D] from the state ``start`` (``start_state``).  x keeps its dtype and row stride; the loop
        enqueues only.  Without ``means`` nothing of n D doubles is allocated."""
        D, dev = self.D, self.device
        n = int(x.shape[0])
        ldx = x.stride(0) if n > 1 else D
        per_pass = plan_blocks(n, D, chunk_bytes)
        slots = int(self.lib.mvnseq_work_len(D, per_pass))
        assert slots == work_slots(D, per_pass)
        work = torch.empty(slots, dtype=torch.float64, device=dev)
        carry = torch.zeros(D * D + D + 1, dtype=torch.float64, device=dev)
        start_d = torch.as_tensor(np.ascontiguousarray(start, dtype=np.float64)).to(dev)
        out = {k: torch.empty((n, D) if k == "means" else n, dtype=torch.float64, device=dev) for k in OUTPUTS if k in want}
        ptr = {k: (out[k].data_ptr() if k in out else None) for k in OUTPUTS}
        blocks = block_count(n)
        self.passes = 0
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            for b in range(0, blocks, per_pass):
                begin, end = block_start(n, b), block_start(n, min(b + per_pass, blocks))
                _check(self.lib.mvnseq_pass(D, _code(x.dtype), x.data_ptr(), ldx, n, begin, end - begin, start_d.data_ptr(),
                                            carry.data_ptr(), ptr["means"], D, ptr["logdet"], ptr["quad"], ptr["nats"],
                                            work.data_ptr(), stream), "mvnseq_pass")
                self.passes += 1
        self.carry = carry
        self.launch_info = f"mvnseq_pass x {self.passes} ({per_pass} blocks of up to {BLOCK} rows each)"
        return out

    def close(self):
        pass
