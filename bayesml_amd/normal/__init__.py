"""Normal model with a Normal-Gamma prior: drop-in for ``bayesml.normal`` whose pass over an array sample runs on the
MI355X (``csrc/expfam_kernels.h``)."""
from ._normal import GenModel, LearnModel

__all__ = ["GenModel", "LearnModel"]
