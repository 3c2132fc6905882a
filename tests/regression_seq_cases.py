"""Late-feature samples for the precision tests of sequential prediction (TEST INFRASTRUCTURE; needs no GPU).

The block form of DESIGN.md 4f is well conditioned once Lambda_c = Lambda_0 + G is: K = I + Z Z^T then has entries of
order one.  A regressor that is zero for the leading rows of a call and switches on later keeps one direction of Lambda_c at
the prior's precision however many rows have been seen; under a diffuse prior the block in which it switches on has K_ii
of 1e6 and more with Schur complements of order one, exactly as a block of the first 2 D rows has.  Everything here is
about that block (the "onset block"):

* seeded recipes (``make``), D = 8 and n = 209 rows of ``regression_oracle.synth_linreg``, noise precision 2:
    late column   column 3 is zero for the rows before 100 (seed 4); y = x theta + the recipe's noise on the changed rows
    late dummy    column 2 is the indicator of row >= 70 (seed 5); y stays that of the unchanged regressors, so the
                  indicator explains nothing of it
    control       the late column under the default prior Lambda_0 = I, which bounds K_ii by 1 + |w|^2: unaffected
* ``onset_block``: the rows of the schedule's block in which the feature switches on.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import regression_oracle as orc
import regression_seq_oracle as seq

D, N, TAU = 8, 209, 2.0
NAMES = ("late column", "late dummy", "control")


@dataclass
class Case:
    name: str
    x: np.ndarray           # [N, D] float64
    y: np.ndarray           # [N] float64
    start: tuple            # (mu_0, Lambda_0, alpha_0, beta_0)
    onset: int              # the first row at which the late feature is not zero

    @property
    def onset_block(self):
        bounds = seq.schedule(len(self.y))
        b = int(np.searchsorted(bounds, self.onset, side="right")) - 1
        return slice(bounds[b], bounds[b + 1])


def make(name: str) -> Case:
    if name not in NAMES:
        raise ValueError(name)
    diffuse = name != "control"
    start = (np.zeros(D), np.eye(D) * (1e-6 if diffuse else 1.0), 1.0, 1.0)
    if name == "late dummy":
        x, y, _theta = orc.synth_linreg(D, N, 5, TAU, np.float64)
        x = x.copy()
        x[:, 2] = np.arange(N) >= 70
        return Case(name, x, y, start, 70)
    x, y, theta = orc.synth_linreg(D, N, 4, TAU, np.float64)
    noise = y - x @ theta
    x = x.copy()
    x[:100, 3] = 0.0
    return Case(name, x, x @ theta + noise, start, 100)
