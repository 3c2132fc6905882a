"""Exponential model with a Gamma prior: drop-in for ``bayesml.exponential`` whose pass over an array sample runs on the
MI355X (``csrc/expfam_kernels.h``)."""
from ._exponential import GenModel, LearnModel

__all__ = ["GenModel", "LearnModel"]
