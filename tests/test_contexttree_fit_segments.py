"""``contexttree.LearnModel.update_posterior(x, lengths=...)`` on the host: what is refused before any engine is opened,
and the C ABI of include/ctfit.h without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

X = np.array([0, 1, 1, 0, 1, 0])


def _model(**kw):
    from bayesml_amd import contexttree
    m = contexttree.LearnModel(2, 2, **kw)
    m._eng = lambda: pytest.fail("the engine was opened")
    return m


@pytest.mark.parametrize("lengths", [[3, 2], [7, -1], [[3, 3]], [3.0, 3.0], np.array([2.5, 3.5])],
                         ids=["sum", "negative", "2-D", "floats", "float-array"])
def test_lengths_are_refused_before_the_engine_is_opened(lengths):
    from bayesml_amd._exceptions import DataFormatError
    with pytest.raises(DataFormatError, match="lengths must be"):
        _model().update_posterior(X, lengths=lengths)


def test_sparse_tables_refuse_two_sequences():
    with pytest.raises(NotImplementedError, match='tables="dense"'):
        _model(tables="sparse").update_posterior(X, lengths=[3, 0, 3])


def test_a_valid_call_needs_the_gpu():
    if torch.cuda.is_available():
        return                              # (an unmarked test does not touch the device)
    from bayesml_amd import contexttree
    from bayesml_amd._engine import EngineUnavailableError
    with pytest.raises(EngineUnavailableError):
        contexttree.LearnModel(2, 2).update_posterior(X, lengths=[3, 3])


def test_ctfit_header_library_and_table_agree():
    from bayesml_amd import _ctfit
    from test_capi_symbols import header_functions
    lib = _ctfit.load_library()
    assert sorted(_ctfit.SYMBOLS) == header_functions("ctfit.h", "ctfit") and lib.ctfit_abi_version() == 1
    assert lib.ctfit_work_len(2, 3) > 0 and lib.ctfit_work_len(2, 30) == -1 and lib.ctfit_head_len(0) == -1
    p = ctypes.c_void_p(4096)               # never dereferenced: the call is refused on its arguments
    assert lib.ctfit_count(_ctfit._CODES[torch.uint8], p, 10, p, p, 2, 0, 2, 2, p, p, p, None) == 1
    assert b"n, S and H must be >= 1" in lib.ctfit_last_error()
    assert np.array_equal(_ctfit.head_offsets([0, 0, 1, 4, 9], 3), [0, 0, 1, 4, 7])
