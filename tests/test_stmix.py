"""The Student-t mixture log-density on the CPU: the NumPy restatement of the kernels' form (tests/stmix_oracle.py) against the
exact oracle inside the derived bound B_i and against scipy, the branch every recipe is there for, the C ABI of
include/stmix.h without a GPU, and the models' host logic through the ``_stmix_pass_factory`` seam.

Measured here (worst |error| / B_i of the restatement, no factor): 0.02 (all_far_below) to 0.14 (nu_across_lgamma_threshold)
over the eleven recipes of tests/stmix_cases.py.
"""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import stmix_cases as cases
import stmix_oracle as so
from conftest import ROOT

_cache = {}


def recipe(name):
    """(case, exact oracle about the default pivot), made once and shared."""
    if name not in _cache:
        c = cases.RECIPES[name]()
        _cache[name] = (c, so.exact(c["u"], c["mu"], c["nu"], c["pi"], c["x"][0], c["x"]))
    return _cache[name]


def args(c):
    return c["x"], c["pi"], c["mu"], c["nu"], c["u"]


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.RECIPES)
def test_restatement_is_inside_the_bound(name):
    c, o = recipe(name)
    lnp, z = so.restate(*args(c))
    worst, at = o.ratio(lnp)
    print(f"{name}: worst |error| / B_i = {worst:.3f} at row {at}")
    assert worst <= 1.0
    decided = o.z_decided()
    assert decided.any() and np.array_equal(z[decided], o.z[decided])


@pytest.mark.parametrize("name", cases.RECIPES)
def test_restatement_against_scipy(name):
    from scipy.special import logsumexp
    from scipy.stats import multivariate_t
    c, o = recipe(name)
    lnp, _ = so.restate(*args(c))
    terms = []
    for k in range(len(c["pi"])):
        uk = np.tril(c["u"][k])
        inv = np.linalg.inv(uk)
        terms.append(np.log(c["pi"][k]) + multivariate_t(loc=c["mu"][k], shape=inv @ inv.T, df=c["nu"][k]).logpdf(c["x"]))
    ref = logsumexp(np.array(terms), axis=0)
    own = np.abs(ref - o.lnp)                                  # scipy's own error, from the oracle
    print(f"{name}: scipy's own error up to {own.max():.1e}, restatement - scipy up to {np.abs(lnp - ref).max():.1e}")
    assert np.all(own <= 1e-6 * (1.0 + np.abs(o.lnp)))         # (1e-7 relative at nu = 1e8: two lgammas of 1e9 subtracted)
    assert np.all(np.abs(lnp - ref) <= o.B + own)


# ---- every recipe takes its branch ----------------------------------------------------------------------------------------
def test_recipes_take_their_branches():
    from bayesml_amd import _stmix
    for name in cases.RECIPES:
        c, o = recipe(name)
        if name != "all_far_below":
            assert o.q[1, 0] == 0.0 and o.q[2, -1] == 0.0, name            # rows exactly at a mean
            assert np.array_equal(c["x"][1], c["mu"][0]) and np.array_equal(c["x"][2], c["mu"][-1])
    c, o = recipe("nu_across_lgamma_threshold")
    half = 0.5 * c["nu"]
    assert (half < _stmix.LGAMMA_SERIES_FROM).sum() == 2 and (half >= _stmix.LGAMMA_SERIES_FROM).sum() == 2
    assert half[2] == _stmix.LGAMMA_SERIES_FROM and c["nu"][0] == 1.0 and c["nu"][3] == 1e8
    c, o = recipe("outliers")
    assert (o.q / c["nu"][None]).max() >= 1e12
    c, o = recipe("all_far_below")
    assert o.t.max() < -1e5 and np.all(np.isfinite(so.restate(*args(c))[0]))
    c, o = recipe("tiny_weights")
    assert c["pi"].min() == 1e-300
    c, o = recipe("cond1e6")
    assert np.linalg.cond(np.tril(c["u"][0]).T @ np.tril(c["u"][0])) > 1e5
    c, o = recipe("far_means")
    assert np.abs(c["mu"]).min() > 9e5
    with_pivot, _ = o.ratio(so.restate(*args(c))[0])
    without, _ = o.ratio(so.restate(*args(c), pivot=np.zeros(16))[0])
    print(f"far_means: |error| / B_i = {with_pivot:.3f} about row 0, {without:.3g} about the origin")
    assert with_pivot <= 1.0 < without                                     # the pivot is what keeps the bound


def test_lgamma_step_keeps_its_digits():
    """lnGamma(a + h) - lnGamma(a) against mpmath at both sides of the threshold and far above it, where two lgamma calls
    subtracted lose seven digits."""
    from bayesml_amd import _stmix
    mp = so.orc._mp()
    for h in (0.5, 8.0, 64.0):
        a = np.array([0.5, 3.0, 63.5, 64.0, 1e3, 5e7, 1e12])
        got = _stmix.lgamma_step(torch.from_numpy(a), h).numpy()
        want = np.array([float(mp.loggamma(mp.mpf(v) + h) - mp.loggamma(mp.mpf(v))) for v in a])
        scale = np.abs(want) + np.array([float(abs(mp.loggamma(mp.mpf(v)))) for v in a]) * (a < 64)
        assert np.all(np.abs(got - want) <= 8 * so.EPS * (1.0 + scale)), (h, got, want)
    naive = float(torch.lgamma(torch.tensor(5e7 + 64.0, dtype=torch.float64)) - torch.lgamma(torch.tensor(5e7, dtype=torch.float64)))
    exact = float(mp.loggamma(mp.mpf(5e7) + 64) - mp.loggamma(mp.mpf(5e7)))
    assert abs(naive - exact) > 1e3 * abs(float(_stmix.lgamma_step(torch.tensor([5e7], dtype=torch.float64), 64.0)[0]) - exact)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree():
    from bayesml_amd import _stmix
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/stmix.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(stmix_[a-z0-9_]+)\s*\(", text)))
    lib = _stmix.load_library()
    assert sorted(_stmix.SYMBOLS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.stmix_abi_version() == 1 == int(re.search(r"#define STMIX_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"#define STMIX_MAX_DEGREE (\d+)", text).group(1)) == _stmix.MAX_DEGREE
    assert int(re.search(r"#define STMIX_MAX_COMPONENTS (\d+)", text).group(1)) == _stmix.MAX_COMPONENTS
    for K, D in ((1, 1), (3, 16), (64, 128), (5, 17), (2, 129), (1, 200)):
        assert lib.stmix_image_len(K, D) == _stmix.image_len(K, D) > 0
    assert lib.stmix_image_len(64, 128) == 64 * 9344            # the E-step's image: 36 tile pairs + the bias, in 1-KB pieces
    for K, D in ((0, 4), (4, 0), (65537, 4), (4, 19201)):
        assert lib.stmix_image_len(K, D) == -1


def test_argument_errors_without_a_gpu():
    from bayesml_amd import _stmix
    lib = _stmix.load_library()
    P, odd, odd16 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)          # never dereferenced

    def refused(rc, text):
        assert rc == 1 and text in lib.stmix_last_error().decode(), (rc, lib.stmix_last_error())

    def pack(K=3, D=4, u=P, m=P, pivot=P, img=P):
        return lib.stmix_pack(K, D, u, m, pivot, img, None)

    refused(pack(K=0), "K must be in 1..65536")
    refused(pack(K=65537), "K must be in 1..65536")
    refused(pack(D=0), "D must be in 1..19200")
    refused(pack(D=19201), "D must be in 1..19200")
    for null in ("u", "m", "pivot", "img"):
        refused(pack(**{null: None}), "null pointer")
    for name in ("u", "m", "pivot"):
        refused(pack(**{name: odd}), "8-byte aligned")
    refused(pack(img=odd16), "img_dev must be 16-byte aligned")

    def logpdf(K=3, D=4, xt=0, x=P, ldx=4, n=10, pivot=P, img=P, c=P, nu=P, lnp=P, z=P):
        return lib.stmix_logpdf(K, D, xt, x, ldx, n, pivot, img, c, nu, lnp, z, None)

    refused(logpdf(K=0), "K must be in 1..65536")
    refused(logpdf(D=0), "D must be in 1..19200")
    refused(logpdf(D=19201, ldx=19201), "D must be in 1..19200")
    refused(logpdf(xt=2), "x_dtype")
    refused(logpdf(n=0), "n_rows")
    refused(logpdf(ldx=3), "ldx")
    for null in ("x", "pivot", "img", "c", "nu", "lnp"):
        refused(logpdf(**{null: None}), "null pointer")
    refused(logpdf(xt=1, x=odd), "aligned to its element size")
    for name in ("pivot", "c", "nu", "lnp", "z"):
        refused(logpdf(**{name: odd}), "8-byte aligned")
    refused(logpdf(img=odd16), "img_dev must be 16-byte aligned")


# ---- the models on the stand-in -------------------------------------------------------------------------------------------
def gmm(K=3, D=2, seed=0):
    """A model with a posterior that is not the prior's, set by hand (no data pass on the CPU)."""
    from bayesml_amd import gaussianmixture as gm
    rng = np.random.default_rng(seed)
    m = gm.LearnModel(K, D, seed=0, verbose=False)
    a = rng.standard_normal((K, D, D))
    m.set_hn_params(hn_alpha_vec=rng.uniform(1.0, 5.0, K), hn_m_vecs=3.0 * rng.standard_normal((K, D)), hn_kappas=rng.uniform(1.0, 9.0, K),
                    hn_nus=D + rng.uniform(0.0, 20.0, K), hn_w_mats=a @ a.transpose(0, 2, 1) + np.eye(D))
    m._stmix_pass_factory = so.StandIn
    return m


def model_oracle(m, x):
    p = m.get_p_params()
    return so.exact_from_precision(p["p_lambda_mats"], p["p_mu_vecs"], p["p_nus"], m.hn_alpha_vec / m.hn_alpha_vec.sum(), x)


@pytest.mark.parametrize("K, D", ((3, 2), (4, 17)))
def test_gaussianmixture_on_the_stand_in(K, D):
    m = gmm(K, D)
    x = 3.0 * np.random.default_rng(5).standard_normal((60, D))
    before = pickle.dumps((m.get_hn_params(), m.hn_w_mats_inv, m._engine, m.r_vecs))
    m.p_nus[:] = -1.0                                          # stale on purpose: the call refreshes them
    lnp = m.calc_pred_logpdf(x)
    want, cond = model_oracle(m, x)
    assert isinstance(lnp, np.ndarray) and lnp.dtype == np.float64 and lnp.shape == (60,)
    assert np.all(np.abs(lnp - want) <= so.model_tolerance(D, cond, want))
    fresh = gmm(K, D).calc_pred_dist()
    for key, val in fresh.get_p_params().items():
        assert np.array_equal(val, m.get_p_params()[key]), key
    assert np.array_equal(fresh.p_pi_vec, m.p_pi_vec)
    assert pickle.dumps((m.get_hn_params(), m.hn_w_mats_inv, m._engine, m.r_vecs)) == before
    # assign
    out = m.calc_pred_logpdf(x, assign=True)
    assert isinstance(out, tuple) and len(out) == 2 and np.array_equal(out[0], lnp)
    z = out[1]
    assert isinstance(z, np.ndarray) and z.dtype == np.int64 and z.shape == (60,) and z.min() >= 0 and z.max() < K
    # a single vector is one row; torch in, torch out; f32 rows
    one = m.calc_pred_logpdf(x[7])
    assert one.shape == (1,) and one[0] == lnp[7]
    tl, tz = m.calc_pred_logpdf(torch.from_numpy(x), assign=True)
    assert isinstance(tl, torch.Tensor) and tl.dtype == torch.float64 and tz.dtype == torch.int64
    assert np.array_equal(tl.numpy(), lnp) and np.array_equal(tz.numpy(), z)
    l32 = m.calc_pred_logpdf(x.astype(np.float32))
    assert l32.dtype == np.float64 and np.array_equal(l32, m.calc_pred_logpdf(x.astype(np.float32).astype(np.float64)))
    assert m.calc_pred_logpdf(x.reshape(6, 10, D)).shape == (60,)
    empty = m.calc_pred_logpdf(np.zeros((0, D)), assign=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0,) and empty[1].dtype == np.int64
    # pickling: the seam is a class, the model holds no engine of this pass
    again = pickle.loads(pickle.dumps(m))
    assert np.array_equal(again.calc_pred_logpdf(x), lnp)


def test_bad_rows_are_refused_with_the_model_untouched():
    from bayesml_amd._exceptions import DataFormatError
    m = gmm()
    m.p_nus[:] = -1.0
    before = pickle.dumps(m.__dict__)
    calls = so.StandIn.calls
    for bad, text in ((np.zeros((4, 3)), "x.shape[-1] must be self.c_degree: x.shape[-1]=3, self.c_degree=2"),
                      (np.zeros((4, 2), dtype=complex), None), (np.array(1.0), None), ([[0.0, 1.0]], None),
                      (torch.zeros(4, 3), "x.shape[-1] must be self.c_degree"), (torch.zeros(4, 2, dtype=torch.int64), "ndim >= 1")):
        with pytest.raises(DataFormatError) as e:
            m.calc_pred_logpdf(bad)
        with pytest.raises(DataFormatError) as e2:
            m._check_rows(bad)
        assert str(e.value) == str(e2.value) and (text is None or text in str(e.value))
    assert pickle.dumps(m.__dict__) == before and so.StandIn.calls == calls


def test_no_gpu_is_an_error_not_a_fallback():
    if torch.cuda.is_available():
        return                              # (an unmarked test does not touch the device)
    from bayesml_amd import gaussianmixture as gm, multivariate_normal as mvn
    from bayesml_amd._engine import EngineUnavailableError
    with pytest.raises(EngineUnavailableError):
        gm.LearnModel(3, 2, verbose=False).calc_pred_logpdf(np.zeros((4, 2)))
    with pytest.raises(EngineUnavailableError):
        mvn.LearnModel(2).calc_pred_logpdf(np.zeros((4, 2)))


@pytest.mark.parametrize("D", (1, 5))
def test_multivariate_normal_on_the_stand_in(D):
    from scipy.stats import multivariate_t
    from bayesml_amd import multivariate_normal as mvn
    from bayesml_amd._exceptions import DataFormatError
    rng = np.random.default_rng(D)
    a = rng.standard_normal((D, D))
    m = mvn.LearnModel(D)
    m.set_hn_params(hn_m_vec=rng.standard_normal(D), hn_kappa=3.0, hn_nu=D + 4.5, hn_w_mat=a @ a.T + np.eye(D))
    m._stmix_pass_factory = so.StandIn
    x = 2.0 * rng.standard_normal((30, D))
    hn = pickle.dumps(m.get_hn_params())
    m.p_nu = -1.0
    lnp = m.calc_pred_logpdf(x)
    assert m.p_nu == m.hn_nu - D + 1 and pickle.dumps(m.get_hn_params()) == hn
    want, cond = so.exact_from_precision(m.p_v_mat[None], m.p_m_vec[None], [m.p_nu], [1.0], x)
    assert lnp.shape == (30,) and np.all(np.abs(lnp - want) <= so.model_tolerance(D, cond, want))
    ref = multivariate_t(loc=m.p_m_vec, shape=m.p_v_mat_inv, df=m.p_nu).logpdf(x)
    assert np.allclose(lnp, ref, rtol=1e-10, atol=1e-10)
    assert m.calc_pred_logpdf(x[3]).shape == (1,)
    t = m.calc_pred_logpdf(torch.from_numpy(x))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), lnp)
    with pytest.raises(TypeError):
        m.calc_pred_logpdf(x, assign=True)
    with pytest.raises(DataFormatError, match="c_degree"):
        m.calc_pred_logpdf(np.zeros((3, D + 1)))
    again = pickle.loads(pickle.dumps(m))
    assert np.array_equal(again.calc_pred_logpdf(x), lnp)
