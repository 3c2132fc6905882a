"""Bayesian linear regression with a Normal-Gamma prior: drop-in for ``bayesml.linearregression`` whose N-sized sums and
per-row predictive parameters run on the MI355X (``csrc/regvb_kernels.h``)."""
from ._linearregression import GenModel, LearnModel

__all__ = ["GenModel", "LearnModel"]
