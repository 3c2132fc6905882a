"""What ``calc_pred_logpdf`` and ``lengths=`` of the regression models refuse before any engine is opened, and the argument
checks of the ``regpred_*`` entry points (include/regpred.h), all without a GPU."""
import ctypes

import numpy as np
import pytest

from bayesml_amd import autoregressive as ar
from bayesml_amd._exceptions import DataFormatError, ParameterFormatError

X = np.arange(12.0)


@pytest.mark.parametrize("lengths", ([5, 6], [13, -1], [[6, 6]], [6.0, 6.0]), ids=("sum", "negative", "2-D", "float"))
@pytest.mark.parametrize("call", ("update_posterior", "calc_pred_logpdf"))
def test_lengths_are_refused_before_the_engine_opens(call, lengths):
    m = ar.LearnModel(2)
    with pytest.raises(DataFormatError, match="lengths must be"):
        getattr(m, call)(X, lengths=np.array(lengths))
    assert m._engine is None and m._score_pass is None


def test_totals_need_lengths_and_a_call_needs_a_row():
    m = ar.LearnModel(3)
    with pytest.raises(ParameterFormatError, match="lengths"):
        m.calc_pred_logpdf(X, totals=True)
    for call in (m.update_posterior, m.calc_pred_logpdf):
        with pytest.raises(DataFormatError, match="greater than self.c_degree"):
            call(X, lengths=[3, 3, 3, 3, 0])                      # no series has more than c_degree values
        with pytest.raises(DataFormatError, match="greater than self.c_degree"):
            call(X[:0], "zeros", lengths=[0, 0])
    assert m._engine is None and m._score_pass is None


def test_regpred_argument_errors_without_a_gpu():
    """Pure argument validation returns error codes before anything touches a device."""
    from bayesml_amd import _regpred, _regression
    lib = _regression.load_library() and _regpred.load_library()
    assert lib.regpred_abi_version() == 1
    assert lib.regpred_work_len(256) == 128 * 16 * 17 and lib.regpred_work_len(257) == -1
    assert lib.regpred_stats_work_len(128) == lib.regvb_stats_work_len(128) and lib.regpred_stats_work_len(0) == -1
    assert lib.regpred_totals_work_len(4097) == 2 and lib.regpred_totals_work_len(0) == 1 and lib.regpred_totals_work_len(-1) == -1
    p = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused on its arguments
    F32, EINVAL, EUNSUPPORTED = 0, 1, 2
    last = lib.regpred_last_error
    post = (p, p, 1.0, 2.0, 0.0, p, p, None)                    # mu, linv, scale, nu, c0, lnp, work, stream
    assert lib.regpred_logpdf(0, F32, p, 4, F32, p, 10, *post) == EINVAL
    assert lib.regpred_logpdf(257, F32, p, 257, F32, p, 10, *post) == EUNSUPPORTED and b"256" in last()
    assert lib.regpred_logpdf(4, 7, p, 4, F32, p, 10, *post) == EINVAL and b"x_dtype" in last()
    assert lib.regpred_logpdf(4, F32, p, 4, 2, p, 10, *post) == EINVAL and b"y_dtype" in last()
    assert lib.regpred_logpdf(4, F32, p, 3, F32, p, 10, *post) == EINVAL and b"ldx" in last()
    assert lib.regpred_logpdf(4, F32, p, 4, F32, p, 0, *post) == EINVAL and b"n_rows" in last()
    assert lib.regpred_logpdf(4, F32, p, 4, F32, p, 10, p, p, 0.0, 2.0, 0.0, p, p, None) == EINVAL and b"scale" in last()
    assert lib.regpred_logpdf(4, F32, p, 4, F32, p, 10, p, p, 1.0, 0.0, 0.0, p, p, None) == EINVAL and b"nu" in last()
    assert lib.regpred_logpdf(4, F32, p, 4, F32, p, 10, p, p, 1.0, 2.0, float("nan"), p, p, None) == EINVAL and b"c0" in last()
    assert lib.regpred_logpdf(4, F32, None, 4, F32, p, 10, *post) == EINVAL and b"null" in last()
    assert lib.regpred_logpdf(4, F32, p, 4, F32, p, 10, p, None, 1.0, 2.0, 0.0, p, p, None) == EINVAL
    assert lib.regpred_logpdf(4, F32, p, 4, 1, ctypes.c_void_p(4100), 10, *post) == EINVAL and b"aligned" in last()
    for fn, tail in ((lib.regpred_logpdf_window, post), (lib.regpred_stats_window, (p, p, None))):
        assert fn(-1, F32, p, 100, 0, 3, p, p, 50, *tail) == EINVAL
        assert fn(256, F32, p, 1000, 0, 3, p, p, 50, *tail) == EUNSUPPORTED
        assert fn(3, 5, p, 100, 0, 3, p, p, 50, *tail) == EINVAL and b"x_dtype" in last()
        assert fn(3, F32, p, 100, 2, 3, p, p, 50, *tail) == EINVAL and b"padding" in last()
        assert fn(3, F32, p, 100, 0, 0, p, p, 50, *tail) == EINVAL and b"n_seq" in last()
        assert fn(3, F32, p, 100, 0, 3, p, p, 0, *tail) == EINVAL and b"n_rows" in last()
        assert fn(3, F32, p, 100, 1, 3, p, p, 101, *tail) == EINVAL and b"n_rows" in last()
        assert fn(3, F32, p, 100, 0, 3, p, None, 50, *tail) == EINVAL and b"null" in last()
    assert lib.regpred_stats_window(3, F32, p, 100, 0, 3, p, p, 50, None, p, None) == EINVAL
    assert lib.regpred_totals(3, p, -1, p, p, None, None, None) == EINVAL
    assert lib.regpred_totals(3, p, 10, p, None, None, None, None) == EINVAL and b"neither" in last()
    assert lib.regpred_totals(0, p, 10, p, p, None, None, None) == EINVAL and b"n_seq" in last()
    assert lib.regpred_totals(3, None, 10, p, p, None, None, None) == EINVAL
    assert lib.regpred_totals(0, None, 10, p, None, p, None, None) == EINVAL and b"null" in last()
