"""ctypes binding of the sequential regression engine of ``libgmmvb.so`` (C ABI in ``include/regseq.h``).

``RegressionSeqPass`` runs ``regseq_pass`` / ``regseq_pass_window`` over a sample pass by pass: every row's Student-t
predictive parameters from the posterior of the rows before it, as n calls of ``LearnModel.pred_and_update`` would give
them, in five launches per pass.  The block schedule belongs to the call; a pass is a range of whole blocks of it, sized by
the workspace budget, and passes carry state only through the ``carry`` statistics block, so the cut changes the workspace
and nothing about the arithmetic.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._native import bind, gpu_device, stream_ptr
from ._regression import MAX_FEATURES, _code, adopt_tensor, check_features

BLOCK = 64                               # include/regseq.h: REGSEQ_BLOCK
DEFAULT_CHUNK_BYTES = 256 << 20
MAX_BLOCKS = (1 << 31) - 1

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/regseq.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "regseq_abi_version": (_int, []),
    "regseq_last_error": (ctypes.c_char_p, []),
    "regseq_block": (_int, [_int]),
    "regseq_block_count": (_i64, [_i64]),
    "regseq_block_start": (_i64, [_i64, _i64]),
    "regseq_work_len": (_i64, [_int, _i64]),
    "regseq_pass": (_int, [_int, _int, _vp, _i64, _int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "regseq_pass_window": (_int, [_int, _int, _vp, _i64, _int, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("regseq", SYMBOLS)


# ---- the schedule and the workspace in Python (csrc/regseq_kernels.h, csrc/regseq.hip: layout_of) ------------------------
def block_count(n: int) -> int:
    """Blocks of the schedule of n rows: lengths 1, 2, 4, ..., BLOCK / 2, then BLOCK, the last one cut at n."""
    if n < BLOCK - 1:
        return int(n).bit_length()
    return BLOCK.bit_length() - 1 + (n - (BLOCK - 1) + BLOCK - 1) // BLOCK


def block_start(n: int, b: int) -> int:
    log2 = BLOCK.bit_length() - 1
    return min(n, (1 << b) - 1 if b <= log2 else BLOCK - 1 + (b - log2) * BLOCK)


def work_slots(D: int, blocks: int) -> int:
    """``regseq_work_len`` in Python, so that passes can be planned without the library."""
    tiles = 2 * ((D + 31) // 32)
    slab = tiles * (tiles + 1) // 2 * 256 + 16 * tiles + 16          # regvb_kernels.h: gram_slab_len
    pd = (D + 15) // 16 * 16
    return blocks + 1 + blocks * (slab + pd * pd + pd + 2)


def plan_blocks(n: int, D: int, chunk_bytes=None) -> int:
    """Blocks per pass: the largest count whose workspace fits ``chunk_bytes`` (1 if none does), at most the schedule's."""
    budget = DEFAULT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    per_block = work_slots(D, 2) - work_slots(D, 1)
    fit = (budget // 8 - 1) // per_block
    return int(max(1, min(fit, block_count(n), MAX_BLOCKS)))


def start_state(mu, lam, alpha, beta):
    """[Lambda_0 | Lambda_0 mu_0 | mu_0^T Lambda_0 mu_0, alpha_0, beta_0] as the passes read it."""
    lam = np.asarray(lam, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    lm = lam @ mu
    return np.concatenate([lam.reshape(-1), lm, [mu @ lm, float(alpha), float(beta)]])


class RegressionSeqPass:
    """The sequential passes for models of D coefficients on one device."""

    def __init__(self, D: int, device):
        check_features(D, "regression")
        self.D = int(D)
        self.lib = load_library()
        self.device = gpu_device(device, "regression data passes")
        assert int(self.lib.regseq_block(self.D)) == BLOCK and D <= MAX_FEATURES
        self.launch_info = ""
        self.passes = 0

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def _run(self, n, call, start, want_nats, chunk_bytes):
        D, dev = self.D, self.device
        per_pass = plan_blocks(n, D, chunk_bytes)
        slots = int(self.lib.regseq_work_len(D, per_pass))
        assert slots == work_slots(D, per_pass)
        work = torch.empty(slots, dtype=torch.float64, device=dev)
        carry = torch.zeros(D * D + D + 2, dtype=torch.float64, device=dev)
        start_d = torch.as_tensor(np.ascontiguousarray(start, dtype=np.float64)).to(dev)
        p_m, p_lambda = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
        nats = torch.empty(n, dtype=torch.float64, device=dev) if want_nats else None
        blocks = block_count(n)
        self.passes = 0
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            for b in range(0, blocks, per_pass):
                begin, end = block_start(n, b), block_start(n, min(b + per_pass, blocks))
                # (p_nu is not asked for: it is 2 alpha_0 + the row index, which the caller has)
                _check(call(begin, end - begin, start_d.data_ptr(), carry.data_ptr(), p_m.data_ptr(), p_lambda.data_ptr(),
                            None, nats.data_ptr() if want_nats else None, work.data_ptr(), stream), "regseq_pass")
                self.passes += 1
        self.launch_info = f"regseq_pass x {self.passes} ({per_pass} blocks of up to {BLOCK} rows each)"
        return p_m, p_lambda, nats

    def run(self, x: torch.Tensor, y: torch.Tensor, start, want_nats: bool, chunk_bytes=None):
        """(p_ms, p_lambdas, nats or None), device tensors [n]: the rows x [n, D] with targets y [n],
        from the state ``start`` (``start_state``).  x and y keep their own dtypes; the loop enqueues only."""
        y = y.contiguous()
        n = int(x.shape[0])
        ldx = x.stride(0) if n > 1 else self.D

        def call(begin, count, *rest):
            return self.lib.regseq_pass(self.D, _code(x.dtype), x.data_ptr(), ldx, _code(y.dtype), y.data_ptr(), n, begin,
                                        count, *rest)
        return self._run(n, call, start, want_nats, chunk_bytes)

    def run_window(self, series: torch.Tensor, padding: int, start, want_nats: bool, chunk_bytes=None):
        """The same for the lag windows of a series (degree D - 1, rows as ``RegressionPass.stats_window``)."""
        p = self.D - 1
        n = int(series.shape[0]) - (0 if padding else p)

        def call(begin, count, *rest):
            return self.lib.regseq_pass_window(p, _code(series.dtype), series.data_ptr(), series.shape[0], int(padding),
                                               begin, count, *rest)
        return self._run(n, call, start, want_nats, chunk_bytes)

    def close(self):
        pass
