"""Seeded samples for the edge tests of multivariate_normal's sequence pass (TEST INFRASTRUCTURE; needs no GPU).

Every recipe returns ``(x, start)`` with ``start = (m_0, kappa_0, nu_0, S_0)``, S_0 = hn_w_mat_inv.  test_mvn_seq_edges.py
holds the NumPy block form to the bound on each of them, test_gpu_mvn_seq_edges.py the kernels.

* ``make`` - the threshold cases (``NAMES``), D = 8 and n = 209 rows of ``mvn_seq_oracle.synth``.  The block form is well
  conditioned once S_c = S_0 + G is: K = I + Z Z^T then has entries of order one.  A coordinate whose innovation is zero
  for the leading rows keeps one direction of S_c at S_0 however many rows have been seen; under S_0 = 1e-6 I the block in
  which it switches on (``onset_block``) has K_ii of 1e6 and more past the first 2 D rows, where only the data can send
  the block to double-double (kDdThreshold).
    late column   column 3 is 0 for the rows before 100 and m_0 = 0: u_3 is exactly 0 until then (seed 502)
    late dummy    column 2 is the indicator of row >= 70 (seed 503)
    control       the late column under S_0 = I, which bounds K_ii by 1 + |u|^2: stays on the matrix pipe
    outlier       x[150] += 1e4 under the default start (seed 504): large K_ii from one row, S_c well conditioned
* ``cut_ns`` - the sample lengths of the cut-block sweep; ``CUTS`` the lengths of the cut block around the waves' edges.
* ``slice_case`` - D from 49 to 256 reaching a whole and a cut block past the first block that starts at or after 2 D rows.
* ``code_length_case`` - the ends of the code length's ranges (``CODE_LENGTH``).
* ``switch_case`` - p_nu / 2 = 64 at row 7 with h = D / 2 = 64 and 128.
"""
import numpy as np

import mvn_seq_oracle as seq

B = seq.BLOCK
D, N = 8, 3 * B + 17
NAMES = ("late column", "late dummy", "control", "outlier")
ONSET = {"late column": 100, "late dummy": 70, "control": 100, "outlier": 150}
CUTS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)       # the waves of a block hold 16 rows each


def diffuse(D):
    return (np.zeros(D), 1.0, float(D), np.eye(D) * 1e-6)


def correlated(D, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((D, D))
    return rng.standard_normal(D) * 0.3, 2.5, D + 1.75, np.eye(D) * 2.0 + a @ a.T / D


# ---- the threshold cases ---------------------------------------------------------------------------------------------------
def make(name):
    if name not in NAMES:
        raise ValueError(name)
    if name == "outlier":
        x = seq.synth(D, N, 504)
        x[150] += 1e4
        return x, seq.default_start(D)
    if name == "late dummy":
        x = seq.synth(D, N, 503)
        x[:, 2] = np.arange(N) >= 70
        return x, diffuse(D)
    x = seq.synth(D, N, 502)
    x[:100, 3] = 0.0
    return x, (seq.default_start(D) if name == "control" else diffuse(D))


def onset_block(name):
    """The rows of the schedule's block that holds the case's onset row, a slice."""
    bounds = seq.schedule(N)
    b = int(np.searchsorted(bounds, ONSET[name], side="right")) - 1
    return slice(bounds[b], bounds[b + 1])


# ---- the cut last block ----------------------------------------------------------------------------------------------------
def cut_ns():
    """Every n up to B + 2 (each ramp block as the cut block; no row, one row and two rows in the first block of 64) and
    B - 1 + L rows for L around every multiple of 16."""
    return tuple(range(1, B + 3)) + tuple(B - 1 + L for L in CUTS)


def cut_case(D):
    return seq.synth(D, 130, 1000 + D), seq.default_start(D)


# ---- the slices of the binary64 K path ---------------------------------------------------------------------------------------
FIRST = {49: 127, 64: 191, 65: 191, 128: 319, 256: 575}
SLICES = [(D_, kind) for D_ in (49, 64, 65, 128, 256) for kind in ("default", "diffuse") if (D_, kind) != (256, "diffuse")]
SLICES += [(64, "correlated"), (128, "correlated")]


def slice_first(D):
    """The first schedule bound at or after 2 D rows."""
    return next(b for b in seq.schedule(4 * D + 2 * B) if b >= 2 * D)


def slice_case(D, kind):
    n = slice_first(D) + B + 17
    start = {"default": seq.default_start, "diffuse": diffuse, "correlated": lambda k: correlated(k, 1200 + k)}[kind](D)
    return seq.synth(D, n, 1100 + D), start


def slice_rows(D):
    """The rows the long-double loop factorises at (None: all): from D = 128 on the first 16, rows 2 D - 4 to 2 D + 4, both
    sides of every block edge from ``first`` on, and every fourth row of the two last blocks counted back from the last."""
    if D < 128:
        return None
    first = slice_first(D)
    n = first + B + 17
    edges = [b for b in seq.schedule(n) if b >= first]
    rows = set(range(16)) | set(range(2 * D - 4, 2 * D + 5)) | {i for e in edges for i in (e - 1, e) if i < n}
    return sorted(rows | set(range(n - 1, first - 1, -4)))


# ---- the ends of the code length's ranges ------------------------------------------------------------------------------------
CODE_LENGTH = ("nu D + 125.5", "nu D + 126", "nu D - 1 + 1e-3", "nu 1e6", "kappa 1e-6", "kappa 1e6", "x 1e-6", "x 1e6",
               "repeated and zero rows", "equal rows", "equal rows diffuse")


def code_length_case(name):
    if name not in CODE_LENGTH:
        raise ValueError(name)
    x = seq.synth(D, N, 1600)
    m, kappa, nu, s = seq.default_start(D)
    if name == "nu D + 125.5":              # a = p_nu / 2 = 63.25 + i / 2 passes 64 between two rows
        nu = D + 125.5
    elif name == "nu D + 126":              # a = 63.5 + i / 2 is 64 exactly at row 1
        nu = D + 126.0
    elif name == "nu D - 1 + 1e-3":         # p_nu = 1e-3 at row 0
        nu = D - 1 + 1e-3
    elif name == "nu 1e6":
        nu = 1e6
    elif name == "kappa 1e-6":
        kappa = 1e-6
    elif name == "kappa 1e6":
        m, kappa = np.full(D, 0.7), 1e6
    elif name == "x 1e-6":
        x = x * 1e-6
    elif name == "x 1e6":
        x = x * 1e6
    elif name == "repeated and zero rows":
        x[100:110] = x[99]
        x[5] = x[64] = 0.0
    elif name == "equal rows":
        x[:] = x[0]
    elif name == "equal rows diffuse":
        x[:] = x[0]
        s = s * 1e-6
    return x, (m, kappa, nu, s)


SWITCH_ROWS = [*range(20), 62, 63, 64]


def switch_case(D):
    """nu_0 = D + 120: p_nu = 121 + i, so a = p_nu / 2 is 64 at row 7, with h = D / 2."""
    return seq.synth(D, B + 1, 600 + D), (np.zeros(D), 1.0, D + 120.0, np.eye(D))


# ---- a second call, passes -----------------------------------------------------------------------------------------------------
def second_call_case():
    return seq.synth(D, N, 1400), diffuse(D)


def strided_case():
    """D = 33 (three slices, a padded last one), to be laid out as f32 rows inside a wider matrix."""
    return seq.synth(33, N, 1500).astype(np.float32), seq.default_start(33)
