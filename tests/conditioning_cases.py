"""Badly conditioned sample matrices for the precision tests of the data pass (TEST INFRASTRUCTURE; needs no GPU).

The engine accumulates raw moments about ONE pivot p (the mean of the leading 4096 rows) and forms
``S_k = B_k/ns_k - a_k a_k^T/ns_k^2`` afterwards; the reference centres each component first
(``_gaussianmixture.py:728-732``).  With ``Delta_k = |x_bar_k - p|`` and ``sigma`` the component's width the engine's
form keeps about ``eps (Delta/sigma)^2`` relative precision of S_k.  Everything here is about that number:

* seeded recipes at ``Delta/sigma ~ R`` (``make``);
* the per-component metric (``per_component``): a broad component must not hide a tight one's error;
* a high-precision reference of the statistics (``reference_stats``: two passes in ``np.longdouble``);
* a NumPy emulation of the engine's formulation (``emulate_engine``): f64 raw moments about the same pivot, summed
  sequentially over row blocks, then ``B/ns - a a^T/ns^2``.  Its error against the reference (the larger one of a few
  block lengths, ``formulation_error``) is what the formulation
  itself costs on a case (``e_emul``); the kernels are held to a small multiple of it (``kernel_bar``).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

RECIPES = ("far", "sorted", "offset", "scales", "flat")
GRID = {np.float32: (1e1, 1e2, 1e3, 1e4), np.float64: (1e1, 1e2, 1e3, 1e4, 1e5)}
OFFSET = {np.float32: 1e4, np.float64: 1e7}
PIVOT_ROWS = 4096                       # the engine's expansion point: mean of the leading rows (_device.py)


@dataclass
class Case:
    recipe: str
    R: float
    dtype: type
    x: np.ndarray           # [N, D] in ``dtype``
    z: np.ndarray           # [N] generating component
    mu: np.ndarray          # [K, D] generating means (f64)
    sd: np.ndarray          # [K, D] generating per-feature standard deviations (0: constant within the component)

    @property
    def name(self):
        return f"{self.recipe}-R{self.R:.0e}-{np.dtype(self.dtype).name}-K{self.mu.shape[0]}-D{self.x.shape[1]}"

    @property
    def pivot(self):
        return pivot_of(self.x)


def pivot_of(x):
    return x[:PIVOT_ROWS].astype(np.float64).mean(axis=0)


def make(recipe: str, R: float, dtype=np.float64, K: int = 4, D: int = 8, N: int = 20_000, seed: int = 0) -> Case:
    """One seeded case.  Means are ``R sigma u_k`` with ``|u_k| ~ 1``, so the clusters sit about ``R sigma`` from each
    other and from the pivot.

    far     K tight clusters (sigma = 1)
    sorted  the rows of ``far`` ordered by label: the leading-rows pivot sits inside the first cluster
    offset  ``far`` plus a common offset of 1e4 (f32) / 1e7 (f64), which the pivot has to absorb; sigma shrinks with R
            (to O / (30 R) once that is below 1) so that the offset is always 30x the spread of the cloud
    scales  clusters in pairs: the pairs R sigma apart, the two clusters of a pair overlapping (about sigma apart);
            then every feature multiplied by its own scale, log-uniform in [1e-3, 1e3]
    flat    ``far`` with feature 0 equal to the label (constant within each component) and the last feature constant
    """
    if recipe not in RECIPES:
        raise ValueError(recipe)
    if recipe == "flat" and D < 3:
        raise ValueError("flat needs D >= 3")
    src = "far" if recipe == "sorted" else recipe
    rng = np.random.default_rng([seed, RECIPES.index(src), int(round(10 * np.log10(R))), K, D, N, np.dtype(dtype).itemsize])
    sigma = 1.0
    if recipe == "offset":
        sigma = min(1.0, OFFSET[dtype] / (30.0 * R))
    u = rng.standard_normal((K, D)) / np.sqrt(D)
    if recipe == "scales":
        pair = rng.standard_normal(((K + 1) // 2, D)) / np.sqrt(D)
        u = pair[np.arange(K) // 2] + u / R            # the two clusters of a pair: about sigma apart
    mu = R * sigma * u
    sd = np.full((K, D), sigma)
    z = rng.integers(0, K, N)
    x = mu[z] + sigma * rng.standard_normal((N, D))
    if recipe == "sorted":
        order = np.argsort(z, kind="stable")
        x, z = x[order], z[order]
    elif recipe == "offset":
        x += OFFSET[dtype]
        mu = mu + OFFSET[dtype]
    elif recipe == "scales":
        c = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), D))
        x *= c
        mu, sd = mu * c, sd * c
    elif recipe == "flat":
        x[:, 0] = z
        mu[:, 0] = np.arange(K)
        const = 0.37 * R * sigma
        x[:, -1] = const
        mu[:, -1] = const
        sd[:, 0] = sd[:, -1] = 0.0
    x = x.astype(dtype)
    return Case(recipe, float(R), dtype, x, z, mu, sd)


def grid(recipes=RECIPES, dtypes=(np.float32, np.float64), max_R=None):
    """(recipe, R, dtype) over the recipes' grid: R up to 1e4 for f32 rows, 1e5 for f64 rows."""
    return [(rc, R, dt) for rc in recipes for dt in dtypes for R in GRID[dt] if max_R is None or R <= max_R]


def responsibilities(case: Case) -> np.ndarray:
    """The generating model's posterior class probabilities (equal weights, axis-aligned Gaussians; features that are
    constant within a component are left out): one-hot for far-apart clusters, soft inside an overlapping pair."""
    x = case.x.astype(np.float64)
    K = case.mu.shape[0]
    lp = np.empty((x.shape[0], K))
    for k in range(K):
        on = case.sd[k] > 0
        d = (x[:, on] - case.mu[k, on]) / case.sd[k, on]
        lp[:, k] = -0.5 * np.sum(d * d, axis=1) - np.sum(np.log(case.sd[k, on]))
    r = np.exp(lp - lp.max(axis=1, keepdims=True))
    return r / r.sum(axis=1, keepdims=True)


# --------------------------------------------------------------------------- statistics
def reference_stats(x, r):
    """The reference's two passes (x_bar_k, then the centred scatter), in np.longdouble -> (ns, x_bar, S) as longdouble.
    Only rows with r_nk > 0 enter component k's scatter (they are the only ones that contribute)."""
    xl = np.asarray(x).astype(np.longdouble)
    rl = np.asarray(r, dtype=np.float64).astype(np.longdouble)
    K, D = rl.shape[1], xl.shape[1]
    ns = rl.sum(axis=0)
    x_bar = np.zeros((K, D), dtype=np.longdouble)
    s = np.zeros((K, D, D), dtype=np.longdouble)
    for k in range(K):
        on = np.asarray(r)[:, k] > 0
        if not on.any():
            continue
        rk, xk = rl[on, k], xl[on]
        x_bar[k] = (rk @ xk) / ns[k]
        d = xk - x_bar[k]
        s[k] = ((rk[:, None] * d).T @ d) / ns[k]
    return ns, x_bar, s


def emulate_engine(x, r, pivot, block: int = 256, acc=np.float64, origin: bool = False):
    """The engine's formulation in NumPy: raw moments ``ns, a = sum r (x - p), B = sum r (x - p)(x - p)^T`` about
    ``pivot`` in ``acc`` precision, summed sequentially over blocks of ``block`` rows, then ``x_bar = p + a/ns`` and
    ``S = B/ns - (a/ns)(a/ns)^T`` in f64.  ``acc=np.float32`` and ``origin=True`` (moments about 0 instead of the pivot)
    are the deliberately broken variants the CPU tests use to show that the kernel-level bar discriminates."""
    p = np.zeros(x.shape[1]) if origin else np.asarray(pivot, dtype=np.float64)
    y = (np.asarray(x, dtype=np.float64) - p).astype(acc)
    r = np.asarray(r, dtype=np.float64).astype(acc)
    N, D = y.shape
    K = r.shape[1]
    ns = np.zeros(K, dtype=acc)
    a = np.zeros((K, D), dtype=acc)
    B = np.zeros((K, D, D), dtype=acc)
    for lo in range(0, N, block):
        yb, rb = y[lo:lo + block], r[lo:lo + block]
        ns += rb.sum(axis=0)
        a += rb.T @ yb
        for k in range(K):
            B[k] += (rb[:, k, None] * yb).T @ yb
    return moments(ns.astype(np.float64), a.astype(np.float64), B.astype(np.float64), p)


def moments(ns, a, B, pivot):
    """(ns, a, B) about ``pivot`` -> (ns, x_bar, S), like ``_kside.moments_from_stats`` (components with ns = 0: zeros)."""
    pos = ns > 0
    safe = np.where(pos, ns, 1.0)
    abar = a / safe[:, None]
    x_bar = np.where(pos[:, None], pivot[None, :] + abar, 0.0)
    s = np.where(pos[:, None, None], B / safe[:, None, None] - abar[:, :, None] * abar[:, None, :], 0.0)
    return ns, x_bar, s


def per_component(q, ref):
    """``max|Q_k - Q_ref,k| / max|Q_ref,k|`` for each component k (leading axis), evaluated in long double."""
    ref = np.asarray(ref).astype(np.longdouble)
    q = np.asarray(q).astype(np.longdouble)
    K = ref.shape[0]
    num = np.abs(q - ref).reshape(K, -1).max(axis=1)
    den = np.abs(ref).reshape(K, -1).max(axis=1)
    return (num / np.where(den > 0, den, 1.0)).astype(np.float64)


def stat_errors(stats, ref):
    """{'ns', 'x_bar', 's'} -> per-component errors of (ns, x_bar, S) against ``reference_stats``."""
    return {key: per_component(q, r) for key, q, r in zip(("ns", "x_bar", "s"), stats, ref)}


EMUL_BLOCKS = (64, 256, 1024)


def formulation_error(x, r, pivot, ref, blocks=EMUL_BLOCKS) -> dict:
    """``e_emul``: per component, the larger error of ``emulate_engine`` over a few block lengths (the kernels sum in
    their own order; one order can be luckier than another by a factor of several)."""
    es = [stat_errors(emulate_engine(x, r, pivot, block=b), ref) for b in blocks]
    return {k: np.maximum.reduce([e[k] for e in es]) for k in es[0]}


def kernel_bar(e_emul: dict, e_ref: dict, floor: float = 1e-12) -> dict:
    """Per component: ``max(100 e_emul, 100 e_ref, floor)`` - as accurate as the formulation allows."""
    return {k: np.maximum(np.maximum(100.0 * e_emul[k], 100.0 * e_ref[k]), floor) for k in e_emul}


def oracle_stats(x, r):
    """The oracle's f64 two-pass statistics (``oracle.gmm_vb_oracle.m_step_stats``, the reference's formulation)."""
    from oracle import gmm_vb_oracle as orc
    return orc.m_step_stats(np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64))
