"""The data pass on far-apart, tight, offset, badly scaled and flat clusters (tests/conditioning_cases.py), against a
long-double two-pass reference and the oracle, every comparison PER COMPONENT.

Kernel level: the statistics of one M-step (ns, x_bar = p + a/ns, S = B/ns - a a^T/ns^2) are as accurate as the
engine's single-pivot formulation allows: per component within ``max(100 e_emul, 100 e_ref, 1e-12)``
(``conditioning_cases.kernel_bar``; ``tests/test_conditioning_cpu.py`` shows that an f32 accumulator or moments about the
origin fail it).  E-step and proof round against the oracle's ln rho; the driver (dense, default and forced sparse
policies, row tiles, the small-problem launch, a 100-iteration fit, the HMM, multivariate_normal) against the oracle's
fit: within 1e-8 per component for R <= 1e3 and within the 1e-5 contract everywhere on the grid."""
import os
import warnings

import numpy as np
import pytest
import torch

import conditioning_cases as cc
from oracle import gmm_vb_oracle as orc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
POLICIES = {"dense": {"GMMVB_ESTEP_PRUNE": "0", "GMMVB_MSTEP_SPARSE": "0"}, "default": {},
            "force": {"GMMVB_ESTEP_PRUNE": "force"}}
ENV_KEYS = ("GMMVB_ESTEP_PRUNE", "GMMVB_MSTEP_SPARSE", "BAYESML_AMD_TILE_ROWS")
_REF = {}


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


def _case(recipe, R, dtype, K=4, D=8, N=20_000):
    """(case, r, long-double reference, e_ref, e_emul), cached over the module."""
    key = (recipe, R, dtype, K, D, N)
    if key not in _REF:
        c = cc.make(recipe, R, dtype, K=K, D=D, N=N)
        r = cc.responsibilities(c)
        ref = cc.reference_stats(c.x, r)
        _REF[key] = (c, r, ref, cc.stat_errors(cc.oracle_stats(c.x, r), ref), cc.formulation_error(c.x, r, c.pivot, ref))
    return _REF[key]


# --------------------------------------------------------------------------- isolated M-step
def _mstep(c, r, prepared):
    from bayesml_amd import _kside
    from bayesml_amd._engine import DataPass
    K, D = r.shape[1], c.x.shape[1]
    xd = torch.from_numpy(c.x).to(DEV)
    eng = DataPass(K, D, xd.dtype, xd.shape[0], DEV)
    try:
        eng.set_pivot(torch.from_numpy(c.pivot).to(DEV))
        if prepared:
            eng.prepare_rows(xd)
        eng.load_responsibilities(torch.from_numpy(r).to(DEV))
        ns, _h, a, B = eng.split_stats(eng.mstep(xd))
        x_bar, s = _kside.moments_from_stats(ns, a, B, eng.pivot, torch.zeros(K, D, D, dtype=torch.float64, device=DEV))
        out = tuple(v.cpu().numpy() for v in (ns, x_bar, s))
        return out, eng.launch_info
    finally:
        eng.close()


def _check_kernel(recipe, R, dtype, K, D, N, forms=(False, True), kernel=None):
    c, r, ref, e_ref, e_emul = _case(recipe, R, dtype, K, D, N)
    bar = cc.kernel_bar(e_emul, e_ref)
    worst = 0.0
    for prepared in forms:
        stats, info = _mstep(c, r, prepared)
        if kernel is not None:
            assert kernel in info, info
        e = cc.stat_errors(stats, ref)
        for key in e:
            assert np.all(e[key] <= bar[key]), (c.name, prepared, key, e[key], e_emul[key], e_ref[key], info)
            worst = max(worst, float(e[key].max()))
    print(f"{c.name} e_engine(S)={worst:.2e} e_emul(S)={e_emul['s'].max():.2e} e_ref(S)={e_ref['s'].max():.2e}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mstep_d8_whole_grid(dtype):
    """One feature tile (T = 1; at K <= 8 several components per wave, mstep_small_f64) over every recipe and R, raw rows
    and the centred copy."""
    for recipe in cc.RECIPES:
        for R in cc.GRID[dtype]:
            _check_kernel(recipe, R, dtype, 4, 8, 20_000, kernel="<T=1")


@pytest.mark.parametrize("D,T", [(64, 4), (128, 8)])
def test_mstep_mfma_tiles(D, T):
    for dtype in (np.float32, np.float64):
        for recipe in ("far", "offset", "scales", "flat"):
            for R in (1e2, 1e4) + ((1e5,) if dtype == np.float64 else ()):
                if D == 128 and recipe == "flat":
                    continue
                _check_kernel(recipe, R, dtype, 4, D, 2048 if D == 64 else 1024, kernel=f"mstep_mfma_f64<T={T}")


@pytest.mark.parametrize("D,kernel", [(160, "mstep_wide_f64"), (300, "mstep_generic_f64")])
def test_mstep_wide_and_generic(D, kernel):
    """At R = 1e2 the bar on S is about 1e-9 (sharp); at the grid's largest R it is 100 e_emul."""
    for dtype in (np.float32, np.float64):
        for recipe in ("far", "offset"):
            for R in (1e2, cc.GRID[dtype][-1]):
                _check_kernel(recipe, R, dtype, 4, D, 1024 if D > 200 else 2048, kernel=kernel)


# --------------------------------------------------------------------------- E-step and proof round
def _posterior(c, r, narrow=False):
    """Oracle posterior after one update from the generating responsibilities, under a prior centred on the data (and,
    ``narrow``, with W0^-1 = the within-component variances: anisotropic U with entries up to 1 / the smallest scale)."""
    x64 = c.x.astype(np.float64)
    K, D = c.mu.shape
    p = orc.Prior.default(K, D)
    p.m[:] = x64.mean(axis=0)
    if narrow:
        v = np.maximum((c.sd ** 2).max(axis=0), 1e-6 * (c.sd ** 2).max())
        p.w[:] = np.diag(1.0 / v)
    p.refresh()
    q = orc.Posterior.from_prior(p)
    ns, x_bar, s = orc.m_step_stats(x64, r)
    orc.update_q_mu_lambda(p, q, orc.Stats(None, r, ns, x_bar, s))
    orc.update_q_pi(p, q, orc.Stats(None, r, ns, x_bar, s))
    return q


def _engine_for(c, q, prepared=True):
    from bayesml_amd import _kside
    from bayesml_amd._engine import DataPass
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=DEV)   # noqa: E731
    qd = _kside.features(_kside.PostT(t(q.alpha), t(q.m), t(q.kappa), t(q.nu), t(q.w_inv)))
    xd = torch.from_numpy(c.x).to(DEV)
    K, D = q.m.shape
    eng = DataPass(K, D, xd.dtype, xd.shape[0], DEV)
    eng.set_pivot(torch.from_numpy(c.pivot).to(DEV))
    if prepared:
        eng.prepare_rows(xd)
    eng.set_params(qd.c, qd.m, qd.u)
    return eng, xd


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_estep_every_recipe(dtype):
    for recipe in cc.RECIPES:
        for R in cc.GRID[dtype]:
            c, r, *_ = _case(recipe, R, dtype)
            q = _posterior(c, r, narrow=recipe == "scales")
            ln_rho, resp = orc.e_step(c.x.astype(np.float64), q)
            eng, xd = _engine_for(c, q)
            try:
                eng.estep(xd)
                e_l = cc.per_component(eng.ln_rho().cpu().numpy().T, ln_rho.T)
                e_r = float(np.max(np.abs(eng.responsibilities().cpu().numpy() - resp)))
            finally:
                eng.close()
            # (at R = 1e5 E[Lambda] itself has a condition number ~1e10: the engine's Cholesky whitening and the oracle's
            # inverse differ by a few 1e-11 of the far components' ln rho ~ -1e10.  ``offset``: the dense E-step forms
            # U x - U m without the pivot, so it keeps ~eps |x| / sigma of ln rho - measured 4e-10 at 1e7 sigma)
            bar = 1e-8 if recipe == "offset" else (1e-11 if R <= 1e4 else 1e-10)
            assert e_l.max() < bar and e_r < 1e-9, (c.name, e_l, e_r)
            print(f"{c.name} e_step ln_rho={e_l.max():.2e} r={e_r:.2e}")


@pytest.mark.parametrize("recipe", ["scales", "far"])
def test_proof_round_encloses_the_oracle(recipe):
    """debug_proof (csrc/estep_i8.h) on rows whose features span six decades / clusters up to 1e5 sigma apart, with
    anisotropic, narrow U: lb <= ln rho <= ub for every row and component, no exceptions, and every row gets a bound
    (lb = -inf, "no bound", would satisfy the enclosure vacuously).  Tightness is asserted on ``far`` only: digits taken
    against a row's largest |x - p| leave the 1e-3-scaled features of ``scales`` next to nothing, so the enclosure is wide
    there (measured 3e2 .. 3e8 times |ln rho|) - a cost in pruning, not in correctness."""
    K, D, N = 4, 64, 4096
    for dtype in (np.float32, np.float64):
        for R in cc.GRID[dtype]:
            for narrow in (False, True):
                c = cc.make(recipe, R, dtype, K=K, D=D, N=N)
                q = _posterior(c, cc.responsibilities(c), narrow=narrow)
                ln_rho, _ = orc.e_step(c.x.astype(np.float64), q)
                eng, _xd = _engine_for(c, q)
                try:
                    for k in range(K):
                        ub, lb = eng.debug_proof(k, N)
                        ub, lb = ub.cpu().numpy().astype(np.float64), lb.cpu().numpy()
                        exact = ln_rho[:, k]
                        assert np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)), (c.name, narrow, k)
                        assert np.all(lb <= exact), (c.name, narrow, k, float(np.max(lb - exact)))
                        assert np.all(ub >= exact), (c.name, narrow, k, float(np.max(exact - ub)))
                        if recipe == "far":
                            # the pairs the round exists to decide (other clusters, hundreds of nats down): within a few
                            # per cent at every R (measured <= 7e-3); a row's own component: the width grows about as R
                            # (3e-3, 2e-2, 0.2, 1.4, 1e2 relative from R = 1e1 to 1e5), so it is held only up to R = 1e2
                            own = c.z == k
                            gap = (ub - lb) / (np.abs(exact) + 1.0)
                            assert gap[~own].max() < 3e-2, (c.name, narrow, k, float(gap[~own].max()))
                            if R <= 1e2:
                                assert gap[own].max() < 5e-2, (c.name, narrow, k, float(gap[own].max()))
                finally:
                    eng.close()


def test_carried_bounds_on_badly_scaled_rows():
    """The loop of test_gpu_sparse_parity.test_carried_bounds_are_upper_bounds_of_the_oracle on a ``scales`` case under
    the forced sparse policy: carried values are exact or upper bounds 80 ln 2 below the row's best; responsibilities
    and per-component statistics equal the oracle's."""
    from bayesml_amd import _kside
    from bayesml_amd import gaussianmixture as gm
    K, D, N = 8, 64, 24_000
    c = cc.make("scales", 1e3, np.float32, K=K, D=D, N=N)
    x64 = c.x.astype(np.float64)
    with _env(POLICIES["force"]):
        m = gm.LearnModel(K, D, seed=0, device=DEV, verbose=False)
        eng, xd = m._open(c.x)
    prior = m._prior_tensors(DEV)
    q = m._init_subsampling(eng, xd, _kside.post_from_prior(prior), N)
    s = torch.zeros(K, D, D, dtype=torch.float64, device=DEV)
    ns, x_bar, s, _h = m._pass(eng, xd, q, s)
    checked = 0
    for it in range(12):
        q_new = _kside.update_q(prior, ns, x_bar, s)
        hint = m._drift_hint(eng, xd, q, q_new)
        assert hint is not None
        before = eng.pass_counts()["estep_sweep"]
        q = q_new
        ns, x_bar, s, _h = m._pass(eng, xd, q, s, hint=(*hint, float((hint[0] - hint[1] / 30.0).min())))
        if eng.pass_counts()["estep_sweep"] == before:
            continue
        lb = eng.ln_rho().cpu().numpy()
        n = lambda t: t.detach().cpu().numpy().copy()   # noqa: E731
        oq = orc.Posterior(alpha=n(q.alpha), m=n(q.m), kappa=n(q.kappa), nu=n(q.nu), w=n(q.w), w_inv=n(q.w_inv))
        oq.refresh_pi()
        oq.refresh_lambda()
        st = orc.data_pass(x64, oq)
        la = st.ln_rho
        same = np.abs(la - lb) <= 1e-8 * np.maximum(1.0, np.abs(la))
        assert np.all(lb[~same] >= la[~same]), (it, "a carried value is not an upper bound")
        mx = la.max(axis=1, keepdims=True)
        lse = mx + np.log(np.exp(la - mx).sum(axis=1, keepdims=True))
        assert np.all((lb <= lse - 55.4) | same), it          # 80 ln 2 = 55.45
        assert np.max(np.abs(eng.responsibilities().cpu().numpy() - st.r)) < 1e-9
        assert cc.per_component(ns.cpu().numpy(), st.ns).max() < 1e-10
        live = st.ns > 0           # (an empty component keeps its previous S in the engine, zeros in this oracle call)
        assert cc.per_component(s.cpu().numpy()[live], st.s[live]).max() < 1e-9, it
        checked += 1
    assert checked >= 3, eng.pass_counts()


# --------------------------------------------------------------------------- driver
HN = (("hn_alpha_vec", "alpha"), ("hn_m_vecs", "m"), ("hn_kappas", "kappa"), ("hn_nus", "nu"), ("hn_w_mats", "w"))


def _bar(R):
    return 1e-8 if R <= 1e3 else 1e-5


def _oracle_fit(x, K, iters):
    D = x.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return orc.update_posterior(x.astype(np.float64), orc.Prior.default(K, D), orc.Posterior.from_prior(orc.Prior.default(K, D)),
                                    np.random.default_rng(0), max_itr=iters, num_init=1, tolerance=0.0)


def _fit(x, K, iters, env, tiles=None):
    from bayesml_amd import gaussianmixture as gm
    with _env(dict(env, **({} if tiles is None else {"BAYESML_AMD_TILE_ROWS": str(tiles)}))):
        m = gm.LearnModel(K, x.shape[1], seed=0, device=DEV, verbose=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.update_posterior(x, max_itr=iters, num_init=1, tolerance=0.0)
    return m


def _check_fit(m, ref, R, what):
    hn = m.get_hn_params()
    for key, attr in HN:
        e = cc.per_component(hn[key], getattr(ref.posterior, attr))
        assert e.max() < _bar(R), (what, key, e)
    return max(float(cc.per_component(hn[k], getattr(ref.posterior, a)).max()) for k, a in HN)


DRIVER = [("far", 1e1, np.float32), ("far", 1e3, np.float32), ("far", 1e4, np.float32), ("far", 1e3, np.float64),
          ("far", 1e5, np.float64), ("sorted", 1e2, np.float32), ("sorted", 1e4, np.float64), ("flat", 1e3, np.float32),
          ("flat", 1e5, np.float64)]


@pytest.mark.parametrize("recipe,R,dtype", DRIVER)
def test_driver_policies_follow_the_oracle(recipe, R, dtype):
    """update_posterior under the dense, default and forced sparse policies at D = 64.  At N K = 80 000 pairs the default
    policy keeps to the dense kernels (it prunes from 2^23 pairs on), so it repeats the dense check here; the forced policy
    runs pruned E-steps and the list M-step (asserted from the pass counts)."""
    K, D, N, iters = 4, 64, 20_000, 8
    c = cc.make(recipe, R, dtype, K=K, D=D, N=N)
    ref = _oracle_fit(c.x, K, iters)
    for tag, env in POLICIES.items():
        m = _fit(c.x, K, iters, env)
        err = _check_fit(m, ref, R, (c.name, tag, m._engine.launch_info))
        counts = m._engine.pass_counts()
        print(f"{c.name} {tag}: {err:.2e} | {counts} | {m._engine.launch_info}")
        if tag == "force":
            assert counts["estep_bound"] + counts["estep_sweep"] >= 1 and counts["mstep_list"] >= 1, counts


def test_driver_row_tiles():
    c = cc.make("sorted", 1e3, np.float32, K=4, D=64, N=20_000)
    ref = _oracle_fit(c.x, 4, 6)
    m = _fit(c.x, 4, 6, {}, tiles=6016)
    assert type(m._engine).__name__ == "TiledDataPass" and m._engine.n_tiles == 4
    _check_fit(m, ref, 1e3, "tiles")


def test_small_fit_far_apart():
    """gmmvb_small_fit (csrc/small.hip) at K = 3, D = 2, N = 1000, R = 1e4."""
    for dtype in (np.float32, np.float64):
        c = cc.make("far", 1e4, dtype, K=3, D=2, N=1000)
        ref = _oracle_fit(c.x, 3, 20)
        m = _fit(c.x, 3, 20, {})
        assert m._small_r is not None                   # the small-problem launch ran
        _check_fit(m, ref, 1e4, ("small", c.name))


@pytest.mark.parametrize("recipe", ["far", "scales"])
def test_hundred_iterations_through_the_settled_row_cache(recipe):
    """The reference's default length under the forced sparse policy (at a test-sized N the default policy stays dense,
    and the cache of single-component rows only exists in pruned passes): the cache's sums are updated incrementally,
    rows entering with weight +1 and leaving with -1 (csrc/mstep.h), for 100 iterations.  On ``scales`` the passes carry
    their bounds (sweeps) and every row ends up settled; on ``far`` the policy takes a fresh bound pass every iteration,
    and the list M-step still takes the single-component rows from the cache (active - accumulated pairs).  Posterior and
    final statistics per component against the oracle."""
    K, D, N, iters = 4, 64, 8000, 100
    c = cc.make(recipe, 1e3, np.float32, K=K, D=D, N=N)
    ref = _oracle_fit(c.x, K, iters)
    m = _fit(c.x, K, iters, POLICIES["force"])
    counts, wk = m._engine.pass_counts(), m._engine.work()
    print(f"{c.name} 100 iterations: {counts} | {wk}")
    assert counts["estep_dense"] == 0 and counts["mstep_list"] >= 90, counts          # pruned passes, list M-steps
    assert wk["active"] - wk["accumulated"] > 0.1 * N, wk                             # the last pass used the cache
    if recipe == "scales":
        assert counts["estep_sweep"] >= 50 and wk["settled_rows"] > 0.5 * N, (counts, wk)
    _check_fit(m, ref, 1e3, ("100 iterations", c.name))
    live = ref.stats.ns > 0
    assert cc.per_component(m.ns, ref.stats.ns).max() < 1e-8
    assert cc.per_component(m.s_mats[live], ref.stats.s[live]).max() < 1e-8
    assert cc.per_component(m.x_bar_vecs[live], ref.stats.x_bar[live]).max() < 1e-8


def test_hmm_sticky_far_apart_states():
    from oracle import hmm_vb_oracle as hov
    from bayesml_amd import hiddenmarkovnormal as hmm
    K, D, T, R = 4, 8, 6000, 1e3
    rng = np.random.default_rng(5)
    mu = R * rng.standard_normal((K, D)) / np.sqrt(D)
    z = np.empty(T, dtype=np.int64)
    z[0] = 0
    u, jump = rng.random(T), rng.integers(0, K, T)
    for t in range(1, T):
        z[t] = z[t - 1] if u[t] < 0.98 else jump[t]
    x = mu[z] + rng.standard_normal((T, D))
    p = hov.HmmPrior.default(K, D)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = hov.update_posterior(x, p, hov.HmmPosterior.from_prior(p), np.random.default_rng(0), max_itr=10, num_init=1,
                                   tolerance=0.0)
        m = hmm.LearnModel(K, D, seed=0, device=DEV, verbose=False)
        m.update_posterior(x, max_itr=10, num_init=1, tolerance=0.0)
    hn = m.get_hn_params()
    for key, attr in (("hn_eta_vec", "eta"), ("hn_zeta_vecs", "zeta"), ("hn_m_vecs", "m"), ("hn_kappas", "kappa"),
                      ("hn_nus", "nu"), ("hn_w_mats", "w")):
        e = cc.per_component(hn[key], getattr(ref.posterior, attr))
        assert e.max() < 1e-8, (key, e)


def test_multivariate_normal_with_shifted_leading_rows():
    """The pivot is the mean of the leading 4096 rows: here they sit 1e4 sigma away from the other rows."""
    from oracle import mvn_oracle
    from bayesml_amd import multivariate_normal as mvn
    D, N = 8, 12_000
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, D))
    x[:cc.PIVOT_ROWS] += 1e4 * rng.standard_normal(D) / np.sqrt(D)
    m = mvn.LearnModel(D, device=DEV)
    m.update_posterior(x)
    rm, rk, rn, rw, rwi = mvn_oracle.update(np.zeros(D), 1.0, float(D), np.eye(D), x)
    e = {k: cc.per_component(a[None], b[None])[0] for k, a, b in (("m", m.hn_m_vec, rm), ("w_inv", m.hn_w_mat_inv, rwi),
                                                                  ("w", m.hn_w_mat, rw))}
    assert m.hn_kappa == rk and m.hn_nu == rn
    assert max(e.values()) < 1e-5, e
