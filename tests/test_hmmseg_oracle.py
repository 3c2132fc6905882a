"""The exact oracle of the many-sequence forward-backward pass (tests/hmmseg_oracle.py) and its derived bound, without a GPU:
the oracle against the reference's recursions, and the reference's recursions in binary64 - a legitimate implementation in
another summation order - inside ONE times the bound on every exact-oracle case of tests/hmmseg_cases.py (the device is held
to twice).  The inputs here are the NumPy emission's ln rho, taken as exact like the engine's are on the device."""
import numpy as np
import pytest

import hmmseg_cases as cases
import hmmseg_oracle as ho
from oracle import hmm_vb_oracle as orc


def test_one_segment_agrees_with_the_reference_recursions():
    K, T = 3, 9
    q, x = cases.random_posterior(K, cases.D), cases.rows(K, T, seed=1)
    ln_rho = orc.emission_ln_rho(x, q)
    o = ho.exact(ln_rho, q.pi_tilde, q.a_tilde, [0, T])
    rho = np.exp(ln_rho - ln_rho.max(axis=1, keepdims=True))
    al, be, c = orc.forward_backward(rho, q.pi_tilde, q.a_tilde)
    xi = al[:-1, :, None] * q.a_tilde[None] * (rho[1:] * be[1:] / c[1:, None])[:, None, :]
    assert np.max(np.abs(o.alpha - al)) < 1e-12 and np.max(np.abs(o.gamma - al * be)) < 1e-12
    assert np.max(np.abs(o.cprime / c - 1.0)) < 1e-12 and np.max(np.abs(o.xi[1:] - xi)) < 1e-12 and np.all(o.xi[0] == 0.0)
    assert np.max(np.abs(o.ms - xi.sum(axis=0))) < 1e-12
    assert np.max(np.abs(o.g0 - o.gamma[0])) == 0.0 and np.max(np.abs(o.gl - o.gamma[-1])) == 0.0
    assert abs(float(o.lnc) - (np.log(c) + ln_rho.max(axis=1)).sum()) < 1e-12 * abs(float(o.lnc))


@pytest.mark.parametrize("name", cases.EXACT_NAMES)
def test_binary64_recursions_stay_inside_the_bound(name):
    case = cases.EXACT[cases.EXACT_NAMES.index(name)]
    x, q, off, _ = cases.inputs(case)
    assert x.shape[0] <= 170 and case["K"] ** 2 * x.shape[0] <= 3e5
    ln_rho = orc.emission_ln_rho(x, q)
    o = ho.exact(ln_rho, q.pi_tilde, q.a_tilde, off)
    r = o.ratios(ho.binary64(ln_rho, q.pi_tilde, q.a_tilde, off))
    print(f"{name}: worst |error| / bound " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + f"; small-entry share {o.small_share:.4f}; smallest product {o.guard:.3g}; min ln rho' {o.d_min:.1f}")
    assert max(r.values()) <= 1.0, r
    assert o.small_share <= 0.01
    assert o.guard > 1e-250, "a product of the recursions comes near the underflow the bound's derivation excludes"
    if case.get("prior"):                                          # the exact zeros are there, and only where they must be
        first = off[:-1][np.diff(off) > 0]
        assert np.all(o.z_alpha[first, 1]) and np.all(o.z_gamma[first, 1]) and o.z_alpha.sum() == len(first)
        assert o.z_ms[2, 0] and o.z_ms[2, 3] and o.z_ms.sum() == 2 and 0.0 < o.ms[2, 1] < 1e-30
        assert not o.z_g0.all() and o.z_g0[1] and not o.z_gl.any()
