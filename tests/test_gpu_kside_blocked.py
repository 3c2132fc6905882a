"""The blocked (16 x 16, f64 MFMA) factor / inverse / W' path of gmmvb_kside_step and gmmvb_kside_factor for D > 32
(csrc/kside.hip: blocked_cholesky, blocked_tri_inverse) at the shapes where the blocking can go wrong: the first D of the
wide path, one below / on / above a block edge, the last partial block; the narrow path (D <= 32) beside it; a badly
conditioned W'^-1 judged by residuals."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POST_FIELDS = ("alpha", "m", "kappa", "nu", "w_inv", "w", "u", "u_inv", "e_ln_pi", "e_ln_lambda_det", "ln_b_w_nu", "c")


def _stepper(prior, pivot, K, D, want_drift, fused):
    from bayesml_amd import _kside
    os.environ["BAYESML_AMD_KSIDE_FUSED"] = "1" if fused else "0"
    os.environ["BAYESML_AMD_KSIDE_GRAPH"] = "0"
    try:
        return _kside.KStepper(prior, pivot, K * (2 + D + D * D), want_drift)
    finally:
        os.environ.pop("BAYESML_AMD_KSIDE_FUSED", None)
        os.environ.pop("BAYESML_AMD_KSIDE_GRAPH", None)


def _random_stats(K, D, n, rng, dev, dead=()):
    x = rng.standard_normal((n, D)) * 1.3 + 0.4
    r = rng.dirichlet(np.ones(K) * 0.3, n)
    for k in dead:
        r[:, k] = 0.0
    ns = r.sum(0)
    h = np.where(r > 0, r * np.log(np.where(r > 0, r, 1.0)), 0.0).sum(0)
    a = r.T @ x
    B = np.stack([(x * r[:, k, None]).T @ x for k in range(K)])
    B = 0.5 * (B + B.transpose(0, 2, 1))
    return torch.from_numpy(np.concatenate([ns, h, a.ravel(), B.ravel()])).to(dev)


def _outputs(s, drift):
    out = [s.ns, s.x_bar, s.s, s.s_prev, s.scal] + [getattr(s.q_next, f) for f in POST_FIELDS]
    return out + ([s.gamma, s.delta, s.big_gamma] if drift else [])


def _check_chained_steps(K, D, drift=True):
    """test_gpu_kside.test_fused_step_matches_torch_functions' construction, tolerances and three chained steps (a dead
    component in the second), with a second fused stepper fed the same inputs: its outputs must be the same bits."""
    from bayesml_amd import _kside
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(K * 100 + D)
    a = rng.standard_normal((K, D, D))
    prior = _kside.prior_from_numpy(rng.uniform(0.3, 2.0, K), rng.standard_normal((K, D)), rng.uniform(0.5, 2.0, K),
                                    D + rng.uniform(0.0, 3.0, K), np.linalg.inv(a @ a.transpose(0, 2, 1) + D * np.eye(D)), dev)
    pivot = torch.from_numpy(rng.standard_normal(D)).to(dev)
    fu, fu2, ea = (_stepper(prior, pivot, K, D, drift, f) for f in (True, True, False))
    assert fu._fused and fu2._fused and not ea._fused
    for it in range(3):
        st = _random_stats(K, D, 40 * K + 5 * D, rng, dev, dead=(1,) if it == 1 else ())
        for s in (fu, fu2, ea):
            s.stats.copy_(st)
            s.step()
        tf, gf = fu.read()
        te, ge = ea.read()
        for key in te:
            assert abs(tf[key] - te[key]) <= 1e-10 * max(1.0, abs(te[key])), (it, key, tf[key], te[key])
        for name in ("ns", "x_bar", "s", "s_prev"):
            a, b = getattr(fu, name), getattr(ea, name)
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (it, name)
        for f in POST_FIELDS:
            a, b = getattr(fu.q_next, f), getattr(ea.q_next, f)
            assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), (it, f)
        w = fu.q_next.w
        assert torch.equal(w, w.transpose(1, 2))
        if drift:
            assert abs(gf - ge) <= 1e-9
            for name in ("gamma", "delta", "big_gamma"):
                a, b = getattr(fu, name), getattr(ea, name)
                assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max())), (it, name)
        for i, (a, b) in enumerate(zip(_outputs(fu, drift), _outputs(fu2, drift))):
            assert torch.equal(a, b), (it, i)
        for s in (fu, fu2, ea):
            s.advance()


@pytest.mark.parametrize("D", [33, 47, 48, 49, 64, 65, 113, 127, 128])
def test_block_edge_shapes_match_torch_functions(D):
    _check_chained_steps(3, D)


@pytest.mark.parametrize("D", [16, 17, 32])
def test_narrow_path_unchanged(D):
    _check_chained_steps(3, D)


def ill_conditioned_steppers():
    """K = 4, D = 128; prior W^-1 = Q diag(logspace(-4, 4)) Q^T (eigenvalues spread over 1e8), statistics from 600 rows.
    Returns (fused stepper, eager stepper) after one step from the prior."""
    from bayesml_amd import _kside
    K, D = 4, 128
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4128)
    lam = np.logspace(-4.0, 4.0, D)
    w = np.empty((K, D, D))
    for k in range(K):
        qm, _ = np.linalg.qr(rng.standard_normal((D, D)))
        w[k] = (qm / lam) @ qm.T                        # W = Q diag(1 / lambda) Q^T
        w[k] = 0.5 * (w[k] + w[k].T)
    prior = _kside.prior_from_numpy(rng.uniform(0.3, 2.0, K), rng.standard_normal((K, D)), rng.uniform(0.5, 2.0, K),
                                    D + rng.uniform(0.0, 3.0, K), w, dev)
    pivot = torch.from_numpy(rng.standard_normal(D)).to(dev)
    st = _random_stats(K, D, 600, rng, dev)
    out = []
    for fused in (True, False):
        s = _stepper(prior, pivot, K, D, False, fused)
        s.stats.copy_(st)
        s.step()
        out.append(s)
    torch.cuda.synchronize()
    return out


def residuals(q):
    """(||G G^T - W'^-1||_max / ||W'^-1||_max, ||u' u'^-1 - I||_max, ||W' W'^-1 - I||_max) of a posterior, the products
    formed in extended precision on the host so that the figures are the posterior's own error."""
    ld = np.longdouble
    w_inv, w, u, u_inv = (getattr(q, f).cpu().numpy().astype(ld) for f in ("w_inv", "w", "u", "u_inv"))
    nu = q.nu.cpu().numpy().astype(ld)
    eye = np.eye(w.shape[1], dtype=ld)
    r = [0.0, 0.0, 0.0]
    for k in range(w.shape[0]):
        g = u_inv[k] * np.sqrt(nu[k])
        r[0] = max(r[0], float(np.abs(g @ g.T - w_inv[k]).max() / np.abs(w_inv[k]).max()))
        r[1] = max(r[1], float(np.abs(u[k] @ u_inv[k] - eye).max()))
        r[2] = max(r[2], float(np.abs(w[k] @ w_inv[k] - eye).max()))
    return tuple(r)


# What the column-by-column kernel of the commit before the blocked one and the eager torch path give on these inputs
# (measured once on an MI355X; (unblocked kernel, eager torch) per residual).  The bound is four times the larger of
# the two: the factor covers the different summation order of a blocked algorithm.
RESIDUALS_BEFORE = {
    "g_gt": (5.084134246457449e-16, 5.332552206923777e-16),
    "u_uinv": (2.419397147901403e-16, 2.6942423986264785e-16),
    "w_winv": (4.9381072148024785e-15, 5.171427522321359e-15),
}


def test_badly_conditioned_w_inv_by_residuals():
    """The blocked kernel on the MI355X where the figures above were taken: (4.55e-16, 4.68e-16, 5.77e-15)."""
    fu, _ = ill_conditioned_steppers()
    assert fu._fused
    got = residuals(fu.q_next)
    print("residuals (G G^T, u u^-1, W W^-1):", got)
    for (name, before), r in zip(RESIDUALS_BEFORE.items(), got):
        assert np.isfinite(r) and r <= 4.0 * max(before), (name, r, before)
    w = fu.q_next.w
    assert torch.equal(w, w.transpose(1, 2))


@pytest.mark.parametrize("D", [33, 49, 128])
def test_kside_factor_blocked(D):
    from bayesml_amd import _engine
    dev = torch.device("cuda", 0)
    K = 5
    gen = torch.Generator(device=dev).manual_seed(30 + D)
    a = torch.randn(K, D, D, dtype=torch.float64, device=dev, generator=gen)
    eye = torch.eye(D, dtype=torch.float64, device=dev)
    w_inv = a @ a.transpose(1, 2) + D * eye
    g, g_inv, logdet = _engine.kside_factor(w_inv)
    ref = torch.linalg.cholesky(w_inv)
    assert float((g - ref).abs().max()) < 1e-11 * float(ref.abs().max())
    assert float((g_inv @ ref - eye).abs().max()) < 1e-10
    assert float((logdet - torch.linalg.slogdet(w_inv)[1]).abs().max()) < 1e-10
    assert bool(torch.all(torch.triu(g, 1) == 0.0)) and bool(torch.all(torch.triu(g_inv, 1) == 0.0))
    g2, g_inv2, logdet2 = _engine.kside_factor(w_inv)
    assert torch.equal(g, g2) and torch.equal(g_inv, g_inv2) and torch.equal(logdet, logdet2)
