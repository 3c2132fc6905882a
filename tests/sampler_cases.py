"""Named case recipes of the sampler edge tests, shared by tests/test_sampler_edges.py (CPU: the NumPy restatement and the
checkers against the exact oracle) and tests/test_gpu_sampler_edges.py (the kernels).  TEST INFRASTRUCTURE, needs no GPU.

Emission cases hand the kernel its factors directly (``factors=``), so a case IS (z, mu, A, seed, row0): A lower
triangular, random, diagonal away from 0.  Chain cases are (pi, a_mat) whose chunk maps do not coalesce.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

# ---- emissions ---------------------------------------------------------------------------------------------------------

DISPATCH_D = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)     # launch_grouped's edges, LDS > 64 KB, the limit
ROW_EDGES = (1, 31, 32, 33, 63, 64, 65)


@dataclass
class Emit:
    name: str
    z: np.ndarray          # [n] int64 in [0, K)
    mu: np.ndarray         # [K, D]
    a: np.ndarray          # [K, D, D] lower triangular: x = mu_z + eps A_z
    seed: int
    row0: int = 0

    @property
    def D(self):
        return self.mu.shape[1]

    @property
    def K(self):
        return self.mu.shape[0]


def _rng(*key):
    return np.random.default_rng([20240607, *key])


def factor(rng, D, scale=1.0):
    """A random lower-triangular factor with entries O(scale / sqrt(D)) and a diagonal in scale [0.5, 1.5]."""
    a = np.tril(rng.standard_normal((D, D))) / np.sqrt(D)
    a[np.arange(D), np.arange(D)] = rng.uniform(0.5, 1.5, D)
    return scale * a


def factor_with_condition(rng, D, cond):
    """Lower triangular with singular values log-spaced from 1 down to 1 / cond: the L of an LQ factorisation."""
    q1, q2 = (np.linalg.qr(rng.standard_normal((D, D)))[0] for _ in range(2))
    m = q1 @ np.diag(np.logspace(0, -np.log10(cond), D)) @ q2
    return np.tril(np.linalg.qr(m.T)[1].T)


def dispatch(D, n=70, K=3):
    """K = 3, n = 70 (tiles of 32, 32 and 6 rows), random classes."""
    rng = _rng(1, D)
    return Emit(f"dispatch-D{D}", rng.integers(0, K, n), 4 * rng.standard_normal((K, D)),
                np.stack([factor(rng, D) for _ in range(K)]), seed=1000 + D)


def _runs_model(K, D=8, tag=0):
    rng = _rng(2, K, tag)
    return 4 * rng.standard_normal((K, D)), np.stack([factor(rng, D) for _ in range(K)])


def class_runs():
    """D = 8: row counts around the 32-row tile, hand-built class runs, mostly-empty classes, the K > 8192 fallback."""
    out = []
    mu, a = _runs_model(3)
    for n in ROW_EDGES:
        out.append(Emit(f"one-class-n{n}", np.full(n, 1), mu, a, seed=2000 + n))
        out.append(Emit(f"alternating-n{n}", np.arange(n) % 3, mu, a, seed=2100 + n))
    for border in (31, 32, 33):
        out.append(Emit(f"border-at-{border}", (np.arange(65) >= border).astype(np.int64) * 2, mu, a, seed=2200 + border))
    mu, a = _runs_model(64)
    out.append(Emit("K64-n40", _rng(3).permutation(64)[:40], mu, a, seed=2300))
    return out


def wide_K():
    """K = 8193 with classes {0, 8192} only: gmmvb_sample_emissions_work_bytes gives 0 and the plain kernel runs."""
    K, D, rng = 8193, 8, _rng(4)
    mu, a = np.zeros((K, D)), np.zeros((K, D, D))
    for k in (0, K - 1):
        mu[k], a[k] = 4 * rng.standard_normal(D), factor(rng, D)
    return Emit("K8193", np.where(rng.random(40) < 0.5, 0, K - 1), mu, a, seed=2400)


def scaled(D=37, n=70):
    """Classes at covariance scale 1e-8, 1 and 1e8 with |mu| up to 1e6, and one factor of condition number 1e8.
    (tests/conditioning_cases.py makes sample matrices, not factors: none of its recipes fits here.)"""
    rng = _rng(5, D)
    a = np.stack([factor(rng, D, 1e-4), factor(rng, D), factor(rng, D, 1e4), factor_with_condition(rng, D, 1e8)])
    mu = rng.standard_normal((4, D)) * np.array([1e6, 1.0, 1e3, 1.0])[:, None]
    return Emit("scaled", np.arange(n) % 4, mu, a, seed=2500)


def unit_scale_model(K=4, D=32):
    """The kind of model tests/test_samplers.py draws (|mu| ~ 4, unit covariance), with one centred class."""
    rng = _rng(6, D)
    mu = 4 * rng.standard_normal((K, D))
    mu[0] = 0.0
    return mu, np.stack([factor(rng, D) for _ in range(K)])


def covariance_scaled(scale, n=400, seed=2600):
    """``unit_scale_model`` with every covariance multiplied by ``scale`` (the factors by its square root)."""
    mu, a = unit_scale_model()
    return Emit(f"cov-x{scale:g}", np.arange(n) % mu.shape[0], mu, np.sqrt(scale) * a, seed=seed)


def emission_cases():
    """Every emission case the GPU file runs against 2 B_j; the CPU file holds the NumPy restatement to the same."""
    return [dispatch(D) for D in DISPATCH_D] + class_runs() + [wide_K(), scaled(), covariance_scaled(1e8)]


def spd_model(K, D, tag):
    """(mu, Lambda) for the default-factor path (the library factors Lambda itself)."""
    rng = _rng(7, D, tag)
    lam = np.stack([np.linalg.inv(np.cov(rng.standard_normal((D, 4 * D))) + 0.2 * np.eye(D)) for _ in range(K)])
    return 4 * rng.standard_normal((K, D)), (lam + lam.transpose(0, 2, 1)) / 2


# ---- latent classes ----------------------------------------------------------------------------------------------------

def latent_pis():
    rng = _rng(8)
    big = rng.dirichlet(np.ones(8192))
    return {
        "zero-first": np.array([0.0, 0.3, 0.7]),
        "zero-middle": np.array([0.4, 0.0, 0.6]),
        "zero-last": np.array([0.25, 0.75, 0.0]),
        "one-hot": np.array([0.0, 0.0, 1.0, 0.0]),
        "ties": np.array([0.25, 0.0, 0.0, 0.25, 0.5, 0.0]),          # equal entries in the cumulative distribution
        "K1": np.array([1.0]),
        "K2": np.array([0.5, 0.5]),
        "K8192": big,
    }


# ---- chains ------------------------------------------------------------------------------------------------------------

CHAIN_T = (1, 2, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 65536 + 257)
LONG_T = 2 ** 24 + 1029             # 65541 chunks, 257 groups: the second trip of the group loop
GROUPS_T = 3 * 65536 + 257          # four groups: the first length at which the state carried from group to group decides


def cyclic_shift(K):
    """s -> s + 1 (mod K) with probability 1: every chunk map is a rotation, non-trivial whenever K does not divide 256."""
    return np.full(K, 1.0 / K), np.roll(np.eye(K), 1, axis=1)


def two_closed_classes():
    rng = _rng(9)
    a = np.zeros((6, 6))
    a[:3, :3], a[3:, 3:] = rng.dirichlet(np.ones(3), 3), rng.dirichlet(np.ones(3), 3)
    return np.array([0.2, 0.1, 0.2, 0.2, 0.2, 0.1]), a


def sticky(stay=1.0 - 1e-4):
    return np.array([0.5, 0.5]), np.array([[stay, 1.0 - stay], [1.0 - stay, stay]])


def cycle_with_jumps(K=5, jump=1e-3):
    a = (1.0 - jump) * np.roll(np.eye(K), 1, axis=1) + jump * np.roll(np.eye(K), 3, axis=1)
    return np.full(K, 1.0 / K), a


def absorbing(p=2e-5):
    """States 0 and 1 swap; either falls into the absorbing state 2 with probability p a step."""
    return np.array([0.5, 0.5, 0.0]), np.array([[0.0, 1.0 - p, p], [1.0 - p, 0.0, p], [0.0, 0.0, 1.0]])


CHAINS = {
    "shift-2": lambda: cyclic_shift(2),              # the swap: a full chunk is the identity, which is not constant either
    "shift-5": lambda: cyclic_shift(5),
    "shift-257": lambda: cyclic_shift(257),
    "shift-300": lambda: cyclic_shift(300),
    "two-classes": two_closed_classes,
    "sticky-2": sticky,
    "cycle-jumps-5": cycle_with_jumps,
    "absorbing": absorbing,
}
LONG_CHAINS = ("cycle-jumps-5", "sticky-2")
# Chains whose GROUP maps (256 chunk maps composed, 65536 steps) do not coalesce either.  The two above do: a sticky or
# jumping chain forgets its start within a group, so thread 0's chaining of the groups could take any state for them.
GROUP_CHAINS = {"shift-5": (GROUPS_T, LONG_T), "shift-257": (GROUPS_T,), "two-classes": (GROUPS_T, LONG_T)}


def chain_seed(name, T):
    return 3000 + 17 * list(CHAINS).index(name) + T
