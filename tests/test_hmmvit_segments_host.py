"""``estimate_latent_vars(x, ..., lengths=...)``: what is refused before an engine is opened (``EngineUnavailableError`` without a GPU)."""
import numpy as np
import pytest

from bayesml_amd import CriteriaError, DataFormatError, ParameterFormatError
from bayesml_amd import hiddenmarkovnormal as hmm
from test_capi_symbols import header_functions


@pytest.mark.parametrize("viterbi", [True, False])
@pytest.mark.parametrize("lengths", [[3, 4], [11, -1], [[5, 5]]])
def test_lengths_are_validated(lengths, viterbi):
    with pytest.raises(DataFormatError):
        hmm.LearnModel(3, 2, seed=0).estimate_latent_vars(np.zeros((10, 2)), "0-1", viterbi, lengths=lengths)


def test_more_than_64_states_with_many_sequences_is_refused():
    with pytest.raises(ParameterFormatError, match="64 states"):
        hmm.LearnModel(65, 2, seed=0).estimate_latent_vars(np.zeros((10, 2)), lengths=[4, 6])
    assert "hmmvb_viterbi_segments" in header_functions()


def test_the_loss_is_checked_first():
    with pytest.raises(CriteriaError):
        hmm.LearnModel(3, 2, seed=0).estimate_latent_vars(np.zeros((10, 2)), "squared", viterbi=True, lengths=[4, 6])
