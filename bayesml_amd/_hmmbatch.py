"""ctypes binding of the HMM predictive of many sequences of ``libgmmvb.so`` (C ABI in ``include/hmmbatch.h``).

``HmmBatchPass`` evaluates ``ln p(x_t | x_0 .. x_{t-1})`` of the rows of S independent sequences laid end to end, the
filtered arg-max paths, each sequence's last filtered posterior and the per-sequence sums: the read-out behind
``hiddenmarkovnormal.LearnModel.calc_pred_logpdf(x, lengths=...)`` ("Predictive log-density of many sequences").
Offsets and the walking order are made here with NumPy and uploaded once; sequences of ``ROUTE_ROWS`` rows and more (up to
64 states) go one by one through ``_hmmpred.HmmFilterPass`` - the chunk-parallel filter is the right tool for them -, every
run of shorter ones between them through ``hmmbatch_logpdf``.  No CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _hmmpred, _stmix
from ._exceptions import DataFormatError, ParameterFormatError
from ._native import bind, gpu_device, stream_ptr
from ._regression import _code, adopt_tensor

MAX_DEGREE = 19200                       # include/hmmbatch.h: HMMBATCH_MAX_DEGREE
MAX_STATES = 256                         # include/hmmbatch.h: HMMBATCH_MAX_STATES
MFMA_STATES = 64                         # include/hmmbatch.h: HMMBATCH_MFMA_STATES
SHEAF = 16                               # include/hmmbatch.h: HMMBATCH_SHEAF
ROUTE_ROWS = 4096                        # _hmmpred.default_plan: from here on a sequence is filtered chunk-parallel

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# every symbol include/hmmbatch.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "hmmbatch_abi_version": (_int, []),
    "hmmbatch_last_error": (ctypes.c_char_p, []),
    "hmmbatch_scratch_len": (_i64, [_int, _int, _i64, _i64]),
    "hmmbatch_logpdf": (_int, [_int, _int, _int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp,
                               _vp, _vp, _vp, _vp]),
    "hmmbatch_totals": (_int, [_i64, _vp, _vp, _vp, _vp]),
}

load_library, _check = bind("hmmbatch", SYMBOLS)


def scratch_len(K: int, D: int, n_rows: int, n_seq: int = 1) -> int:
    """``hmmbatch_scratch_len`` in Python (csrc/hmmbatch.hip: layout): rho' [npad][Kp], m [npad], ln e [K][npad]."""
    kp = 16 * ((K + 15) // 16)
    npad = (n_rows + 63) // 64 * 64
    return npad * kp + npad + npad * K


def sequence_offsets(lengths, n: int) -> np.ndarray:
    """``lengths`` as the S + 1 row offsets of the sequences of a sample of n rows (host int64), checked on the host as
    ``contexttree.LearnModel._sequence_offsets`` does it."""
    msg = "lengths must be a 1-dimensional array, tensor or list of non-negative integers whose sum is the number of rows of x"
    if hasattr(lengths, "detach"):
        lengths = lengths.detach().cpu().numpy()
    try:
        arr = np.asarray(lengths)
    except Exception:
        raise DataFormatError(msg) from None
    if isinstance(lengths, (list, tuple)) and arr.size == 0:
        arr = arr.astype(np.int64)
    if arr.ndim != 1 or arr.dtype.kind not in "iu" or (arr.size and int(arr.min()) < 0):
        raise DataFormatError(msg)
    off = np.concatenate([[0], np.cumsum(arr.astype(np.int64))]).astype(np.int64)
    if int(off[-1]) != n:
        raise DataFormatError(msg)
    return off


def plan_segments(K: int, D: int, off: np.ndarray, chunk_bytes: int) -> list:
    """The calls of a batch, in sequence order: ``("batch", s_lo, s_hi)`` = the sequences s_lo .. s_hi - 1 in one
    ``hmmbatch_logpdf`` whose scratch fits ``chunk_bytes``, ``("single", s, s + 1)`` = one sequence through
    ``HmmFilterPass`` (``ROUTE_ROWS`` rows or more at up to ``_hmmpred.PARALLEL_STATES`` states, or larger than the budget
    on its own: that path slices time)."""
    budget = max(0, int(chunk_bytes)) // 8
    fit = budget // scratch_len(K, D, 64) * 64           # the most rows whose scratch fits: the scratch grows by 64 rows
    lens = np.diff(off)
    single = lens > fit
    if K <= _hmmpred.PARALLEL_STATES:
        single |= lens >= ROUTE_ROWS
    stops = np.append(np.flatnonzero(single), len(lens))      # the singles, and the end
    segs, s, S = [], 0, len(lens)
    while s < S:
        if single[s]:
            segs.append(("single", s, s + 1))
            s += 1
            continue
        # up to the next single, and as many whole sequences as fit (at least this one)
        e = min(int(stops[np.searchsorted(stops, s)]), int(np.searchsorted(off, off[s] + fit, side="right")) - 1)
        segs.append(("batch", s, e))
        s = e
    return segs


class HmmBatchPass:
    """The batch pass for HMMs of K states with Student-t emissions in D dimensions on one device."""

    def __init__(self, K: int, D: int, device):
        _hmmpred.check_shape(K, D)
        self.K, self.D = int(K), int(D)
        _stmix.load_library()                # (stmix_pack's prototype: the parameter image is its)
        self.lib = load_library()
        self.device = gpu_device(device, "HMM batch predictive")
        self.img = torch.empty(int(self.lib.stmix_image_len(self.K, self.D)), dtype=torch.float64, device=self.device)
        self._single = None                  # the HmmFilterPass of the routed sequences, made when one comes
        self.launch_info = ""
        self.last = None

    def adopt(self, a):
        return adopt_tensor(a, self.device)

    def run(self, x: torch.Tensor, off, a, w0, mu, nu, u, want_z: bool, want_tot: bool = False, pivot=None,
            chunk_bytes: int = _hmmpred.DEFAULT_CHUNK_BYTES):
        """(ln p [n] float64, z [n] int64 or None, end [S, K], tot [S] or None) as device tensors for the rows x [n, D]
        (f32 or f64, read where they lie) of the S sequences with host row offsets ``off`` [S + 1], each filtered on its
        own from w0 ([K]: the same for all, or [S, K]) under a, mu, nu, u as ``HmmFilterPass.run`` takes them.  ``pivot``
        [D] defaults to row 0 of x: one pivot for the whole batch.  Enqueues only."""
        K, D, dev = self.K, self.D, self.device
        off = np.ascontiguousarray(off, dtype=np.int64)
        n, S = int(x.shape[0]), len(off) - 1
        assert S >= 1 and off[0] == 0 and off[-1] == n and np.all(np.diff(off) >= 0) and n >= 1
        ldx = x.stride(0) if n > 1 else D
        t = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()      # noqa: E731
        a, w0, mu, nu, u = t(a), t(w0), t(mu), t(nu), t(u)
        assert a.shape == (K, K) and w0.shape in ((K,), (S, K)) and mu.shape == (K, D) and nu.shape == (K,) and u.shape == (K, D, D)
        per_seq = w0.dim() == 2
        pivot = x[0].to(torch.float64).contiguous() if pivot is None else t(pivot)
        c = _stmix.log_norm_consts(torch.ones_like(nu), nu, u)
        segs = plan_segments(K, D, off, chunk_bytes)
        # each batch call's own offsets (from 0) and walking order (longest first, stable), uploaded once
        offs, orders, at = [], [], {}
        for kind, lo, hi in segs:
            if kind == "batch":
                at[lo] = (sum(len(v) for v in offs), sum(len(v) for v in orders))
                offs.append(off[lo:hi + 1] - off[lo])
                orders.append(np.argsort(-np.diff(off[lo:hi + 1]), kind="stable").astype(np.int32))
        off_dev = torch.from_numpy(np.concatenate(offs + [off])).to(dev)          # (the last S + 1: the whole batch's, for tot)
        order_dev = torch.from_numpy(np.concatenate(orders)).to(dev) if orders else None
        rows = max([int(off[hi] - off[lo]) for kind, lo, hi in segs if kind == "batch"], default=0)
        need = int(self.lib.hmmbatch_scratch_len(K, D, rows, 1))
        assert need == scratch_len(K, D, rows)
        scratch = torch.empty(max(need, 2), dtype=torch.float64, device=dev)
        lnp = torch.empty(n, dtype=torch.float64, device=dev)
        z = torch.empty(n, dtype=torch.int64, device=dev) if want_z else None
        end = torch.empty((S, K), dtype=torch.float64, device=dev)
        tot = torch.empty(S, dtype=torch.float64, device=dev) if want_tot else None
        diag = torch.zeros(2, dtype=torch.int64, device=dev)
        ptr = lambda v, i, size: v.data_ptr() + int(i) * size                  # noqa: E731
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            _stmix._check(self.lib.stmix_pack(K, D, u.data_ptr(), mu.data_ptr(), pivot.data_ptr(), self.img.data_ptr(), stream),
                          "stmix_pack")
            for kind, lo, hi in segs:
                r0, r1 = int(off[lo]), int(off[hi])
                if kind == "single":
                    self._run_single(x[r0:r1], a, w0[lo] if per_seq else w0, mu, nu, u, want_z, pivot, chunk_bytes,
                                     dict(lnp=lnp[r0:r1], z=None if z is None else z[r0:r1], end=end[lo], diag=diag))
                    continue
                o_at, q_at = at[lo]
                _check(self.lib.hmmbatch_logpdf(
                    K, D, _code(x.dtype), ptr(x, r0 * ldx, x.element_size()), ldx, r1 - r0, hi - lo, ptr(off_dev, o_at, 8),
                    ptr(order_dev, q_at, 4), pivot.data_ptr(), self.img.data_ptr(), c.data_ptr(), nu.data_ptr(), a.data_ptr(),
                    ptr(w0, lo * K, 8) if per_seq else w0.data_ptr(), K if per_seq else 0, scratch.data_ptr(), ptr(lnp, r0, 8),
                    None if z is None else ptr(z, r0, 8), ptr(end, lo * K, 8), None, stream), "hmmbatch_logpdf")
            if want_tot:                     # one code path for every sequence, the routed ones included
                _check(self.lib.hmmbatch_totals(S, ptr(off_dev, len(off_dev) - S - 1, 8), lnp.data_ptr(), tot.data_ptr(), stream),
                       "hmmbatch_totals")
        # (what the engine was handed: the tests' oracle starts from exactly these)
        self.last = dict(a=a, w0=w0, mu=mu, nu=nu, u=u, pivot=pivot, c=c, off=off, segments=segs,
                         order=[o.copy() for o in orders], chunk_len=0, sweep_len=0)
        n_batch = sum(kind == "batch" for kind, _, _ in segs)
        self.launch_info = (f"hmmbatch_logpdf ({'plain f64' if D > 128 else 'f64 MFMA'} emission, "
                            f"{'f64 MFMA sheaves of 16' if K <= MFMA_STATES else 'a workgroup per sequence'}, K={K}, D={D}, "
                            f"{S} sequences, {n} rows, {n_batch} batch calls, {len(segs) - n_batch} routed)")
        return lnp, z, end, tot

    def _run_single(self, x, a, w0, mu, nu, u, want_z, pivot, chunk_bytes, out):
        """One sequence through ``HmmFilterPass.run`` into the slices ``out``; in time slices - each from the true phi A of
        the slice before - if its scratch does not fit ``chunk_bytes`` (``_hmmpred.model_logpdf``'s rule)."""
        if self._single is None:
            self._single = _hmmpred.HmmFilterPass(self.K, self.D, self.device)
        step = _hmmpred.slice_rows(self.K, self.D, chunk_bytes)
        for lo in range(0, int(x.shape[0]), step):
            part = dict(lnp=out["lnp"][lo:lo + step], z=None if out["z"] is None else out["z"][lo:lo + step], end=out["end"],
                        diag=out["diag"])
            self._single.run(x[lo:lo + step], a, w0, mu, nu, u, want_z, pivot=pivot, out=part)
            w0 = out["end"] @ a

    def close(self):
        pass


# ---- the model's method ---------------------------------------------------------------------------------------------------------
def start_vectors(model, start, S: int) -> np.ndarray:
    """w0 of ``calc_pred_logpdf(x, lengths=...)``: ``_hmmpred.start_vector``'s forms ([K], for every sequence) or an
    [S, K] matrix, a row per sequence, each row checked like the vector."""
    if not isinstance(start, str):
        rows = start.detach().to("cpu") if isinstance(start, torch.Tensor) else start
        try:
            two_d = np.ndim(rows) == 2
        except Exception:
            two_d = False
        if two_d:
            if len(rows) != S:
                raise ParameterFormatError(f"a start matrix must have one row per sequence: {S} rows of c_num_classes weights")
            return np.stack([_hmmpred.start_vector(model, row) for row in rows]) if S else np.zeros((0, model.c_num_classes))
    return _hmmpred.start_vector(model, start)


def model_logpdf(model, x, as_numpy: bool, off, start, want_z: bool, want_state: bool, want_tot: bool, chunk_bytes, params):
    """``calc_pred_logpdf(x, lengths=...)`` of the HMM: the start vectors, the engine, the parameters
    ``params(device) -> (a, mu, nu, u)`` and the return kinds."""
    K, D = model.c_num_classes, model.c_degree
    S = len(off) - 1
    w0 = start_vectors(model, start, S)
    if chunk_bytes is None:
        chunk_bytes = _hmmpred.DEFAULT_CHUNK_BYTES
    if not (isinstance(chunk_bytes, (int, np.integer)) and chunk_bytes > 0):
        raise ParameterFormatError("chunk_bytes must be a positive integer")
    n = int(x.shape[0])
    if n == 0:                                   # nothing was filtered: every state is its start vector
        lnp, z = torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.int64)
        state = torch.from_numpy(np.broadcast_to(w0, (S, K)).copy())
        tot = torch.zeros(S, dtype=torch.float64)
    else:
        eng = HmmBatchPass(K, D, model._device)
        a, mu, nu, u = params(eng.device)
        lnp, z, state, tot = eng.run(eng.adopt(x), off, a, w0, mu, nu, u, want_z, want_tot, chunk_bytes=int(chunk_bytes))
        model._hmmbatch_pass = eng
    out = [lnp] + ([z] if want_z else []) + ([state] if want_state else []) + ([tot] if want_tot else [])
    if as_numpy:
        out = [v.detach().to("cpu").numpy() for v in out]
    return out[0] if len(out) == 1 else tuple(out)
