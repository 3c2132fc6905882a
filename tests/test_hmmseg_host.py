"""``hiddenmarkovnormal.LearnModel.update_posterior(x, lengths=...)``: what is decided or drawn before the device is touched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bayesml_amd import DataFormatError, ParameterFormatError
from bayesml_amd import hiddenmarkovnormal as hmm
from test_capi_symbols import header_functions


@pytest.mark.parametrize("lengths", [[3, 4], [5, 6], [[5, 5]], [5.0, 5.0], [11, -1], "ab"])
def test_lengths_are_validated(lengths):
    with pytest.raises(DataFormatError):
        hmm.LearnModel(3, 2, seed=0).update_posterior(np.zeros((10, 2)), lengths=lengths)


def test_more_than_64_states_with_many_sequences_is_refused():
    m = hmm.LearnModel(65, 2, seed=0)
    with pytest.raises(ParameterFormatError, match="64 states"):
        m.update_posterior(np.zeros((10, 2)), lengths=[4, 6])
    assert m._segment_offsets(np.zeros((10, 2)), [0, 10, 0]) is None          # one non-empty sequence: today's call
    assert "hmmvb_forward_backward_segments" in header_functions()            # (the entry point the others take)


def test_random_responsibility_of_many_sequences():
    K, off = 3, np.array([0, 0, 1, 4, 4, 6])                                  # lengths 0, 1, 3, 0, 2
    draw = np.random.default_rng(5).dirichlet(np.ones(K * K), 6).reshape(6, K, K)
    xi = draw.copy()
    gamma, ms, g0, gl = hmm.LearnModel._random_segments(xi, off)
    assert np.all(xi[[0, 1, 4]] == 0.0) and np.array_equal(xi[[2, 3, 5]], draw[[2, 3, 5]])
    assert np.array_equal(ms, xi.sum(axis=0))
    assert np.array_equal(gamma[0], draw[0].sum(axis=0))                      # one row: its own marginal, before the zeroing
    assert np.array_equal(gamma[1], draw[2].sum(axis=1)) and np.array_equal(gamma[4], draw[5].sum(axis=1))
    assert np.array_equal(gamma[[2, 3, 5]], draw[[2, 3, 5]].sum(axis=1))
    assert np.array_equal(g0, gamma[0] + gamma[1] + gamma[4]) and np.array_equal(gl, gamma[0] + gamma[3] + gamma[5])


def test_random_pass_draws_as_the_single_sequence_call_does():
    K, xd = 3, torch.zeros(6, 2, dtype=torch.float64)
    eng = SimpleNamespace(load_responsibilities=lambda r: None, mstep=lambda x, out=None: None)
    ks = [SimpleNamespace(stats=None, fb=torch.zeros(K * K + 2 * K + 1, dtype=torch.float64)) for _ in range(2)]
    one, many = hmm.LearnModel(K, 2, seed=11), hmm.LearnModel(K, 2, seed=11)
    one._random_pass(eng, xd, ks[0])
    many._random_pass(eng, xd, ks[1], (np.array([0, 1, 4, 6]), None, None))
    assert one.rng.random() == many.rng.random()                              # the same consumption of the Generator
    assert abs(float(ks[0].fb[:K * K].sum()) - 5.0) < 1e-12 and abs(float(ks[1].fb[:K * K].sum()) - 3.0) < 1e-12
