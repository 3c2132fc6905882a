"""Bernoulli model with a Beta prior: drop-in for ``bayesml.bernoulli`` whose pass over an array sample runs on the
MI355X (``csrc/expfam_kernels.h``)."""
from ._bernoulli import GenModel, LearnModel

__all__ = ["GenModel", "LearnModel"]
