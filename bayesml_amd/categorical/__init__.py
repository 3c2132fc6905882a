"""Categorical model with a Dirichlet prior: drop-in for ``bayesml.categorical`` whose pass over an array sample runs on the
MI355X (``csrc/expfam_kernels.h``)."""
from ._categorical import GenModel, LearnModel

__all__ = ["GenModel", "LearnModel"]
