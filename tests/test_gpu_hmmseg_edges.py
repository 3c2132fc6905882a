"""The forward-backward pass over many sequences on the MI355X (csrc/hmmseg_kernels.h, run_segments in csrc/hmm_capi.hip) at
its branch edges (tests/hmmseg_cases.py), against the exact oracle of tests/hmmseg_oracle.py from the ln rho array the engine
holds and the pi~, A~, off it was handed: alpha, gamma, c', every xi read-out, ms, g0, gl and sum ln c within TWICE the derived
bound, exact zeros exactly zero.  Where a batch has too many segments for mpmath the per-segment binary64 oracle stands in, at
the tolerances tests/test_gpu_hmmseg.py already uses (said next to each), with identities that are literal equalities."""
import numpy as np
import pytest

import hmmseg_cases as cases
import hmmseg_oracle as ho
from conftest import rel_err
from test_gpu_hmmseg import batch, random_posterior, segment_oracle, segment_pass

pytestmark = pytest.mark.gpu

_ORACLES = {}


def oracle_of(ln_rho, q, off):
    """The exact oracle of these inputs, computed once per module (cases that differ in the walking order or a developer
    switch alone share it when the engine's ln rho is the same bits)."""
    key = (off.tobytes(), q.pi_tilde.tobytes(), q.a_tilde.tobytes(), ln_rho.tobytes())
    if key not in _ORACLES:
        _ORACLES[key] = ho.exact(ln_rho, q.pi_tilde, q.a_tilde, off)
    return _ORACLES[key]


# K = 1 .. 64: every block count and the steps between them (16 | 17, 32 | 33 - the last count with the xi sum inside the backward
# kernel -, 48 | 49), lengths around kSegAhead and twice it; whole-empty sheaves in sorted and in given order; one long member
# among short ones at either end of the sheaf; a wave that takes three sheaves at one and at two blocks; the w_tm path over an
# empty sheaf; exact zeros in pi~ and A~.
@pytest.mark.parametrize("name", cases.EXACT_NAMES)
def test_against_the_exact_oracle(name, monkeypatch):
    case = cases.EXACT[cases.EXACT_NAMES.index(name)]
    for env in ("GMMVB_DEBUG", case["switch"]) if case.get("switch") else ():
        monkeypatch.setenv(env, "4")
    x, q, off, order = cases.inputs(case)
    r = segment_pass(x, q, off, order=order, pivot=cases.PIVOT)
    o = oracle_of(r["ln_rho"], q, off)
    ratios = o.ratios(r)
    print(f"{name}: worst |error| / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items())
          + f"; small-entry share {o.small_share:.4f}")
    assert max(ratios.values()) <= 2.0, ratios
    assert o.small_share <= 0.01 and o.guard > 1e-250 and r["gate"] == -1
    if case.get("prior"):          # (the zeros are the oracle's: `ratios` asserted them entry by entry; here, that they exist)
        assert o.z_alpha.any() and o.z_gamma.any() and o.z_ms.sum() == 2 and o.z_g0[1] and np.all(r["cprime"] > 0.0)
        assert np.all(r["ms"][o.z_ms] == 0.0) and r["g0"][1] == 0.0


# Every sequence one row, T = S: no transition anywhere.  S = 1, T = 1 at K = 33 launches no xi kernel and reads no slab.
# (binary64 oracle; 1e-10 on alpha, gamma, g0, gl and 1e-9 relative on sum ln c are tests/test_gpu_hmmseg.py's tolerances)
@pytest.mark.parametrize("K, S", cases.ONES)
def test_no_transition_at_all(K, S):
    x, q, off = cases.rows(K, S, seed=K + S), random_posterior(K, cases.D), np.arange(S + 1, dtype=np.int64)
    r, o = segment_pass(x, q, off, pivot=cases.PIVOT), segment_oracle(x, q, off)
    assert np.all(r["ms"] == 0.0) and np.all(r["xi"] == 0.0)
    assert np.array_equal(r["g0"], r["gl"])       # (gamma = alpha o 1 / sum alpha is alpha to rounding only: no bit claim there)
    assert np.max(np.abs(r["alpha"] - o["alpha"])) < 1e-10 and np.max(np.abs(r["gamma"] - o["gamma"])) < 1e-10
    assert np.max(np.abs(r["g0"] - o["g0"])) < 1e-10
    assert abs(r["lnc"] - o["lnc"]) < 1e-9 * max(1.0, abs(o["lnc"])) and abs(r["ns"].sum() - S) < 1e-7


# A second call on one engine after a larger one: fewer sheaves, slabs and partial blocks than the buffers last held.  The
# engine is built for the larger batch and takes the smaller row count after it (DataPass allows that).
@pytest.mark.parametrize("K", cases.REUSE)
def test_a_smaller_batch_on_a_used_engine(K):
    (x1, off1), q = batch(K, cases.D, 65), random_posterior(K, cases.D)
    x2, off2 = cases.rows(K, 5, seed=K), np.arange(6, dtype=np.int64)
    big = segment_pass(x1, q, off1, pivot=cases.PIVOT, keep=True)
    assert big["ms"].sum() > 100.0                                  # (transitions were counted into the slabs)
    try:
        again = segment_pass(x2, q, off2, pivot=cases.PIVOT, eng=big["eng"])
    finally:
        big["eng"].close()
    fresh = segment_pass(x2, q, off2, pivot=cases.PIVOT)
    assert np.array_equal(again["ln_rho"], fresh["ln_rho"])
    for key in ("alpha", "cprime", "gamma", "xi", "ms", "g0", "gl"):
        assert np.array_equal(again[key], fresh[key]), key
    assert again["lnc"] == fresh["lnc"] and np.all(again["ms"] == 0.0)
    assert rel_err(again["ns"], fresh["ns"]) < 1e-9                 # (the M-step's sum, not this entry's: the existing tolerance)


# The g0 / gl reduction: n_part at its cap of 256 with per = 65 and trailing blocks past n_seq, and n_part cut by the room
# for partial sums with all but ten sequences empty.  (binary64 oracle, vectorised over the length classes; tolerances of
# tests/test_gpu_hmmseg.py: 1e-10 on a row's gamma, so 1e-10 per sequence with rows on g0 and gl - their sums are that count,
# which is at most S -, 1e-9 relative on ms and sum ln c, 1e-7 on the two totals.)
@pytest.mark.parametrize("which", ["cap", "room"])
def test_the_ends_reduction(which):
    K, lengths = 3, cases.ends_lengths(which)
    off, S, n_rows = cases.offsets(lengths), len(lengths), int((lengths > 0).sum())
    if which == "cap":
        assert S > 64 * 256 and -(-S // 256) == 65 and 253 * 65 >= S
    else:
        assert n_rows == 10 and -(-S // 64) > cases.room_sequences(int(off[-1]), K)[1]
    x, q = cases.rows(K, int(off[-1]), seed=S), random_posterior(K, cases.D)
    r, o = segment_pass(x, q, off, pivot=cases.PIVOT), cases.batched_oracle(x, q, off)
    assert abs(o["g0"].sum() - n_rows) < 1e-9 * n_rows
    assert np.max(np.abs(r["g0"] - o["g0"])) <= 1e-10 * n_rows and np.max(np.abs(r["gl"] - o["gl"])) <= 1e-10 * n_rows
    assert np.max(np.abs(r["gamma"] - o["gamma"])) < 1e-10 and rel_err(r["ms"], o["ms"]) < 1e-9
    assert abs(r["lnc"] - o["lnc"]) < 1e-9 * max(1.0, abs(o["lnc"]))
    assert abs(r["ns"].sum() - x.shape[0]) < 1e-7 and abs(r["ms"].sum() - (x.shape[0] - n_rows)) < 1e-7
    first = off[:-1][lengths > 0]
    assert np.all(r["xi"][first] == 0.0) and r["gate"] == -1
