"""The HMM predictive of many sequences without a GPU: what ``calc_pred_logpdf(x, lengths=...)`` refuses before any engine
exists, the C ABI of include/hmmbatch.h on bad arguments, and header, library and ctypes table against each other."""
import ctypes
import pickle
import re

import numpy as np
import pytest

from conftest import ROOT
from test_hmmpred import hmm


def _state(m):
    return pickle.dumps((m.get_hn_params(), m.get_p_params(), m._gamma_last, m._hmmbatch_pass))


@pytest.mark.parametrize("kw, error", [
    (dict(lengths=[4, -1, 3]), "DataFormatError"),
    (dict(lengths=[2.5, 3.5]), "DataFormatError"),
    (dict(lengths=[[3, 3]]), "DataFormatError"),
    (dict(lengths=[3, 2]), "DataFormatError"),
    (dict(totals=True), "ParameterFormatError"),
    (dict(lengths=[3, 3], start=np.array([[0.2, 0.3, 0.5], [0.5, 0.6, -0.1]])), "ParameterFormatError"),
    (dict(lengths=[3, 3], start=np.array([[0.2, 0.3, 0.5]])), "ParameterFormatError"),
])
def test_refused_before_an_engine_exists(kw, error):
    from bayesml_amd import _exceptions
    m = hmm(3, 2)
    m.calc_pred_dist()
    before = _state(m)
    with pytest.raises(getattr(_exceptions, error)):
        m.calc_pred_logpdf(np.zeros((6, 2)), **kw)
    assert _state(m) == before and m._hmmbatch_pass is None


def test_no_rows_needs_no_engine():
    m = hmm(3, 2)
    w = np.array([[0.2, 0.3, 0.5], [1.0, 0.0, 0.0]])
    lnp, z, state, tot = m.calc_pred_logpdf(np.zeros((0, 2)), lengths=[0, 0], start=w, assign=True, return_state=True, totals=True)
    assert lnp.shape == z.shape == (0,) and np.array_equal(state, w) and np.array_equal(tot, [0.0, 0.0])


def test_segments_cut_at_sequence_boundaries():
    from bayesml_amd import _hmmbatch
    off = np.concatenate([[0], np.cumsum([7, 4096, 0, 9, 64, 1, 200])])
    assert _hmmbatch.plan_segments(4, 2, off, 1 << 30) == [("batch", 0, 1), ("single", 1, 2), ("batch", 2, 7)]
    assert _hmmbatch.plan_segments(65, 2, off, 1 << 30) == [("batch", 0, 7)]          # (the wide path walks serially anyway)
    budget = 8 * _hmmbatch.scratch_len(4, 2, 128)
    assert _hmmbatch.plan_segments(4, 2, off, budget) == [("batch", 0, 1), ("single", 1, 2), ("batch", 2, 6), ("single", 6, 7)]
    for kind, lo, hi in _hmmbatch.plan_segments(4, 2, off, budget):
        assert kind == "single" or 8 * _hmmbatch.scratch_len(4, 2, int(off[hi] - off[lo])) <= budget


def test_scratch_len_and_argument_errors_without_a_gpu():
    from bayesml_amd import _hmmbatch
    lib = _hmmbatch.load_library()
    for K in (1, 16, 17, 64, 65, 256):
        for n in (0, 1, 63, 64, 65, 10 ** 7):
            assert lib.hmmbatch_scratch_len(K, 3, n, 5) == _hmmbatch.scratch_len(K, 3, n, 5)
    assert lib.hmmbatch_scratch_len(32, 16, 1000, 5) == 1024 * 32 + 1024 + 1024 * 32
    for K, D, n, S in ((0, 3, 10, 1), (257, 3, 10, 1), (3, 0, 10, 1), (3, 19201, 10, 1), (3, 3, -1, 1), (3, 3, 10, 0), (3, 3, 10, 2 ** 31)):
        assert lib.hmmbatch_scratch_len(K, D, n, S) == -1
    P, odd, odd16 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)          # never dereferenced

    def call(K=3, D=4, xt=0, x=P, ldx=4, n=10, S=2, off=P, order=P, pivot=P, img=P, c=P, nu=P, a=P, w0=P, stride=0, scratch=P,
             lnp=P, z=P, end=P, tot=P):
        return lib.hmmbatch_logpdf(K, D, xt, x, ldx, n, S, off, order, pivot, img, c, nu, a, w0, stride, scratch, lnp, z, end, tot,
                                   None)

    def refused(rc, text, code=1):
        assert rc == code and text in lib.hmmbatch_last_error().decode(), (rc, lib.hmmbatch_last_error())

    refused(call(K=0), "K must be >= 1")
    refused(call(K=257), "at most 256 states", code=2)
    refused(call(D=19201, ldx=19201), "D must be in 1..19200")
    refused(call(n=-1), "n_rows")
    refused(call(S=0), "n_seq")
    refused(call(S=2 ** 31), "n_seq")
    refused(call(xt=2), "x_dtype")
    refused(call(ldx=3), "ldx")
    refused(call(stride=2), "w0_stride")
    for null in ("x", "off", "order", "pivot", "img", "c", "nu", "a", "w0", "scratch", "lnp", "end"):
        refused(call(**{null: None}), "null pointer")
    refused(call(xt=1, x=odd), "aligned to its element size")
    for name in ("off", "pivot", "c", "nu", "a", "w0", "lnp", "z", "end", "tot"):
        refused(call(**{name: odd}), "8-byte aligned")
    refused(call(order=ctypes.c_void_p(4098)), "order_dev 4-byte")
    refused(call(img=odd16), "16-byte aligned")
    refused(lib.hmmbatch_totals(0, P, P, P, None), "n_seq")
    refused(lib.hmmbatch_totals(2, None, P, P, None), "null pointer")


def test_header_library_and_ctypes_table_agree():
    from bayesml_amd import _hmmbatch
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/hmmbatch.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hmmbatch_[a-z0-9_]+)\s*\(", text)))
    lib = _hmmbatch.load_library()
    assert sorted(_hmmbatch.SYMBOLS) == declared and len(declared) == 5
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.hmmbatch_abi_version() == 1 == int(re.search(r"#define HMMBATCH_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MAX_DEGREE", _hmmbatch.MAX_DEGREE), ("MAX_STATES", _hmmbatch.MAX_STATES),
                         ("MFMA_STATES", _hmmbatch.MFMA_STATES), ("SHEAF", _hmmbatch.SHEAF)):
        assert int(re.search(rf"#define HMMBATCH_{macro} (\d+)", text).group(1)) == value
