"""The drift kernel's triangular / symmetric tile products (csrc/kside.hip, drift_kernel), the drift combine folded into
kside_finish_kernel, and the single packing launch of gmmvb_set_params (pack_images_kernel).

The drift kernel is held to its torch specification (bayesml_amd._kside._norm2_upper and the delta formula, evaluated
eagerly on the full products) at 1e-9 relative - the tolerance tests/test_gpu_kside.py uses for the same quantities - and
to the singular values themselves: every output is a rigorous bound.  The shapes cover every PD instantiation (32, 64,
128), padding inside a 16 x 16 tile, PD = 32 with idle waves, and exactly full tiles.

Non-finite input: the issue's case puts one NaN into a lower-triangle entry of u_new.  u_new is an operand of the
directions 1 and 2 (big_gamma, enorm) and of delta only; direction 0 multiplies u_old by u_new^-1, so gamma = 0 can only
follow from a NaN in u_new^-1.  A posterior that went non-finite has the NaN in both factors (they come from one
factorisation), so the test runs both: the NaN in u_new alone (big_gamma = enorm = +inf, gamma untouched), and the NaN at
the same entry of u_new and u_new^-1 (gamma = 0 as well).  In both the other components are bit-equal to the clean run."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import gmm_vb_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(3, 7), (5, 16), (4, 33), (3, 64), (3, 65), (2, 100), (2, 128)]
SQUARINGS = [(8, 6), (0, 0), (1, 3)]


def _dev():
    return torch.device("cuda", 0)


def _posterior(K, D, scale, seed=5):
    """The construction of tests/test_gpu_kside.py:91-100: one SPD batch, and a perturbation of it by ``scale``."""
    from bayesml_amd import _kside
    dev = _dev()
    a = torch.randn(K, D, D, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    w_inv = a @ a.transpose(1, 2) + D * torch.eye(D, dtype=torch.float64, device=dev)
    p = torch.randn(K, D, D, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(seed + 2)) * scale
    w_inv = w_inv + p @ p.transpose(1, 2) * D
    m = torch.randn(K, D, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(seed + 1)) + scale
    one = torch.ones(K, dtype=torch.float64, device=dev)
    return _kside.features(_kside.PostT(one.clone(), m, one.clone(), torch.full((K,), D + 2.0, dtype=torch.float64, device=dev), w_inv))


@functools.lru_cache(maxsize=None)
def _pair(K, D, scale=0.03):
    return _posterior(K, D, 0.0), _posterior(K, D, scale)


def _raw(u_old, uinv_old, m_old, u_new, uinv_new, m_new, sq, sq_big):
    """gmmvb_kside_drift itself: (gamma, delta, big_gamma, enorm) as the kernel writes them."""
    from bayesml_amd._engine import _check, _vp, load_library
    lib = load_library()
    K, D = m_old.shape
    t = [x.contiguous() for x in (u_old, uinv_old, m_old, u_new, uinv_new, m_new)]
    out = torch.empty(4, K, dtype=torch.float64, device=m_old.device)
    with torch.cuda.device(m_old.device):
        st = _vp(torch.cuda.current_stream(m_old.device).cuda_stream)
        _check(lib, lib.gmmvb_kside_drift(K, D, *(x.data_ptr() for x in t), int(sq), int(sq_big), out[0].data_ptr(),
                                          out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), st), "gmmvb_kside_drift")
    torch.cuda.synchronize()
    return out


def _raw_q(q0, q1, sq=8, sq_big=6):
    return _raw(q0.u, q0.u_inv, q0.m, q1.u, q1.u_inv, q1.m, sq, sq_big)


@functools.lru_cache(maxsize=None)
def _exact(K, D, scale=0.03):
    """Singular values of u_new u_old^-1, ||u_new u_old^-1 - I||_2 and ||u_new (m_new - m_old)||, on the host."""
    q0, q1 = _pair(K, D, scale)
    b = (q1.u @ q0.u_inv).cpu()
    sv = torch.linalg.svdvals(b)
    e = torch.linalg.svdvals(b - torch.eye(D, dtype=torch.float64))[:, 0]
    d = torch.linalg.vector_norm((q1.u @ (q1.m - q0.m)[:, :, None])[:, :, 0], dim=1).cpu()
    return sv[:, -1], sv[:, 0], e, d


def _rel(a, b):
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("sq,sq_big", SQUARINGS)
@pytest.mark.parametrize("K,D", SHAPES)
def test_drift_matches_the_torch_specification_and_bounds_the_singular_values(K, D, sq, sq_big):
    from bayesml_amd import _kside
    q0, q1 = _pair(K, D)
    gamma, delta, big, enorm = _raw_q(q0, q1, sq, sq_big)
    # 1. the specification, eagerly on the full products
    b = q1.u @ q0.u_inv
    want_gamma = (1.0 - 1e-9) / _kside._norm2_upper(q0.u @ q1.u_inv, sq)
    want_big = (1.0 + 1e-9) * _kside._norm2_upper(b, sq_big)
    want_e = (1.0 + 1e-9) * _kside._norm2_upper(b - torch.eye(D, dtype=b.dtype, device=b.device), sq)
    want_delta = torch.linalg.vector_norm((q1.u @ (q1.m - q0.m)[:, :, None])[:, :, 0], dim=1) * (1.0 + 1e-9)
    for name, got, want in (("gamma", gamma, want_gamma), ("big_gamma", big, want_big), ("enorm", enorm, want_e), ("delta", delta, want_delta)):
        print(name, _rel(got, want))
        assert _rel(got, want) <= 1e-9, name
    # 2. rigour
    smin, smax, e_exact, d_exact = _exact(K, D)
    gamma, delta, big, enorm = (t.cpu() for t in (gamma, delta, big, enorm))
    assert bool(torch.all(gamma <= smin)) and bool(torch.all(big >= smax))
    assert bool(torch.all(enorm >= e_exact)) and bool(torch.all(delta >= d_exact))
    # 3. looseness
    if (sq, sq_big) == (8, 6):
        assert bool(torch.all(gamma >= 0.97 * smin)) and bool(torch.all(big <= 1.05 * smax))


@pytest.mark.parametrize("K,D", SHAPES)
def test_drift_when_the_components_hardly_move_or_do_not_move(K, D):
    from bayesml_amd import _kside
    q0, q1 = _pair(K, D, 1e-6)
    smin, smax, _e, _d = _exact(K, D, 1e-6)
    enorm = _raw_q(q0, q1)[3].cpu()
    assert bool(torch.all(1.0 - enorm <= smin)) and bool(torch.all(1.0 + enorm >= smax))
    out = _raw_q(q0, q0)
    assert bool(torch.isfinite(out).all())
    assert bool(torch.all(out[0] <= 1.0)) and bool(torch.all(out[2] >= 1.0))
    g, d, big = _kside.drift(q0, q0)
    assert bool(torch.isfinite(g).all() and torch.isfinite(d).all() and torch.isfinite(big).all())
    assert bool(torch.all(g <= 1.0)) and bool(torch.all(big >= 1.0))


@pytest.mark.parametrize("K,D", SHAPES)
def test_drift_reads_no_upper_triangle_and_repeats_itself(K, D):
    q0, q1 = _pair(K, D)
    clean = _raw_q(q0, q1)
    assert torch.equal(clean, _raw_q(q0, q1))                      # 7. run to run
    gen = torch.Generator(device=_dev()).manual_seed(11)
    junk = []
    for t in (q0.u, q0.u_inv, q1.u, q1.u_inv):
        assert float(t.triu(1).abs().max()) == 0.0 if D > 1 else True          # (the contract: lower triangular)
        g = torch.randn(K, D, D, dtype=torch.float64, device=_dev(), generator=gen) * 1e3
        junk.append(t + g.triu(1))
    got = _raw(junk[0], junk[1], q0.m, junk[2], junk[3], q1.m, 8, 6)
    assert torch.equal(got, clean)                                   # 5. the strict upper triangles are not read


def test_drift_non_finite_input_is_confined_to_its_component():
    from bayesml_amd import _kside
    K, D, bad = 3, 40, 1
    q0, q1 = _pair(K, D)
    clean = _raw_q(q0, q1)
    others = [k for k in range(K) if k != bad]
    u_nan = q1.u.clone()
    u_nan[bad, 17, 5] = float("nan")
    # the NaN in u_new alone: the directions that read u_new give up, gamma (u_old u_new^-1) does not see it
    out = _raw(q0.u, q0.u_inv, q0.m, u_nan, q1.u_inv, q1.m, 8, 6)
    assert float(out[2, bad]) == float("inf") and float(out[3, bad]) == float("inf")
    assert torch.equal(out[0], clean[0])
    assert torch.equal(out[:, others], clean[:, others])
    # ... and in both factors, as a posterior that went non-finite has it; as the wrapper sees it
    uinv_nan = q1.u_inv.clone()
    uinv_nan[bad, 17, 5] = float("nan")
    out = _raw(q0.u, q0.u_inv, q0.m, u_nan, uinv_nan, q1.m, 8, 6)
    assert float(out[0, bad]) == 0.0 and float(out[2, bad]) == float("inf") and float(out[3, bad]) == float("inf")
    assert torch.equal(out[:, others], clean[:, others])
    qn = _kside.PostT(q1.alpha, q1.m, q1.kappa, q1.nu, q1.w_inv)
    qn.u, qn.u_inv = u_nan, uinv_nan
    g, d, big = _kside.drift(q0, qn)
    g0, d0, big0 = _kside.drift(q0, q1)
    assert float(g[bad]) == 0.0 and float(big[bad]) == float("inf")
    assert torch.equal(g[others], g0[others]) and torch.equal(d[others], d0[others]) and torch.equal(big[others], big0[others])


# ---- the fused step with the combine folded into kside_finish_kernel --------------------------------------------------
def _steppers(K, D, seed):
    from bayesml_amd import _kside
    dev = _dev()
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((K, D, D))
    prior = _kside.prior_from_numpy(rng.uniform(0.3, 2.0, K), rng.standard_normal((K, D)), rng.uniform(0.5, 2.0, K),
                                    D + rng.uniform(0.0, 3.0, K), np.linalg.inv(a @ a.transpose(0, 2, 1) + D * np.eye(D)), dev)
    pivot = torch.from_numpy(rng.standard_normal(D)).to(dev)
    out = []
    for fused in ("1", "0"):
        os.environ["BAYESML_AMD_KSIDE_FUSED"] = fused
        os.environ["BAYESML_AMD_KSIDE_GRAPH"] = "0"
        try:
            out.append(_kside.KStepper(prior, pivot, K * (2 + D + D * D), True))
        finally:
            os.environ.pop("BAYESML_AMD_KSIDE_FUSED", None)
            os.environ.pop("BAYESML_AMD_KSIDE_GRAPH", None)
    return out, rng, dev


def _random_stats(K, D, n, rng, dev):
    x = rng.standard_normal((n, D)) * 1.3 + 0.4
    r = rng.dirichlet(np.ones(K) * 0.3, n)
    ns = r.sum(0)
    h = np.where(r > 0, r * np.log(np.where(r > 0, r, 1.0)), 0.0).sum(0)
    a = r.T @ x
    B = np.stack([(x * r[:, k, None]).T @ x for k in range(K)])
    B = 0.5 * (B + B.transpose(0, 2, 1))
    return torch.from_numpy(np.concatenate([ns, h, a.ravel(), B.ravel()])).to(dev)


@pytest.mark.parametrize("K,D", [(3, 40), (4, 128)])
def test_fused_step_with_drift_matches_the_eager_stepper(K, D):
    (fu, ea), rng, dev = _steppers(K, D, K * 100 + D)
    assert fu._fused and not ea._fused
    for it in range(3):                         # chained: q_next of one step is the q of the next
        st = _random_stats(K, D, 40 * K + 5 * D, rng, dev)
        for s in (fu, ea):
            s.stats.copy_(st)
            s.step()
        tf, gf = fu.read()
        te, ge = ea.read()
        for key in te:
            assert abs(tf[key] - te[key]) <= 1e-10 * max(1.0, abs(te[key])), (it, key, tf[key], te[key])
        assert abs(gf - ge) <= 1e-9, (it, gf, ge)
        for name in ("gamma", "delta", "big_gamma"):
            a, b = getattr(fu, name), getattr(ea, name)
            assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max())), (it, name)
        for s in (fu, ea):
            s.advance()


# ---- the packing launch: the images it writes, through fits held to the oracle ------------------------------------------
ENV_KEYS = ("GMMVB_ESTEP_PRUNE", "GMMVB_MSTEP_SPARSE", "BAYESML_AMD_SMALL")


class _env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ENV_KEYS}
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _rel_np(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def _fit_against_oracle(K, D, N, env):
    """Three VB iterations of the public driver against the oracle's, at tests/test_gpu_sparse_parity.py's tolerances."""
    from bayesml_amd import gaussianmixture as gm
    x = orc.synth_gmm(K, D, N, np.float32)
    with _env(env):
        m = gm.LearnModel(K, D, seed=0, device=_dev(), verbose=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.update_posterior(x, max_itr=3, num_init=1, tolerance=0.0)
        counts = m._engine.pass_counts()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = orc.Prior.default(K, D)
        ref = orc.update_posterior(x.astype(np.float64), p, orc.Posterior.from_prior(p), np.random.default_rng(0), max_itr=3,
                                   num_init=1, tolerance=0.0)
    hn, q = m.get_hn_params(), ref.posterior
    for key, want in (("hn_alpha_vec", q.alpha), ("hn_m_vecs", q.m), ("hn_kappas", q.kappa), ("hn_nus", q.nu), ("hn_w_mats", q.w)):
        assert _rel_np(hn[key], want) < 1e-6, key
    assert _rel_np(m.hn_w_mats_inv, q.w_inv) < 1e-6
    assert _rel_np(m.ns, ref.stats.ns) < 1e-6 and _rel_np(m.x_bar_vecs, ref.stats.x_bar) < 1e-6
    assert _rel_np(m.s_mats, ref.stats.s) < 1e-5
    assert np.max(np.abs(m.r_vecs - ref.stats.r)) < 1e-6
    assert abs(m.vl - ref.vl) <= 1e-8 * abs(ref.vl)
    m._engine.close()
    return counts


@pytest.mark.parametrize("K,D", [(3, 49), (4, 100), (3, 128)])
def test_int8_images_of_the_single_packing_launch(K, D):
    counts = _fit_against_oracle(K, D, 3000, {"GMMVB_ESTEP_PRUNE": "force"})
    assert counts["estep_bound"] >= 1 and counts["estep_gather"] >= 1, counts          # the int8 images were used


@pytest.mark.parametrize("K,D", [(3, 7), (3, 33)])
def test_f64_image_padding_of_the_single_packing_launch(K, D):
    counts = _fit_against_oracle(K, D, 2000, {"GMMVB_ESTEP_PRUNE": "0", "GMMVB_MSTEP_SPARSE": "0", "BAYESML_AMD_SMALL": "0"})
    assert counts["estep_bound"] == 0, counts
