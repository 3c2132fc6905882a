"""Meta-tree forests over mixed continuous and categorical features (``bayesml.metatree``)."""
from ._metatree import GenModel, LearnModel, _Node

__all__ = ["GenModel", "LearnModel"]
