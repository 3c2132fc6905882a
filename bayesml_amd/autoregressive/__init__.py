"""Bayesian autoregressive model with a Normal-Gamma prior: drop-in for ``bayesml.autoregressive`` whose pass over the
series runs on the MI355X (``csrc/regvb_kernels.h``)."""
from ._autoregressive import GenModel, LearnModel

__all__ = ["GenModel", "LearnModel"]
