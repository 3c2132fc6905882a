"""Context tree model: drop-in for ``bayesml.contexttree`` whose posterior update, MAP sweep and counting pass run on the
MI355X (``csrc/ctree_kernels.h``)."""
from ._contexttree import GenModel, LearnModel, _Node

__all__ = ["GenModel", "LearnModel"]
