"""linearregression / autoregressive LearnModel and GenModel: oracle and host logic against reference-generated fixtures
on the CPU (the data passes through tests/fake_regression_engine.py), C-ABI argument validation without a GPU, and every
fixture through the real kernels on the GPU.

Tolerances (rel_err = max|a-b| / max|b|): 1e-10 for hn_lambda_mat, hn_mu_vec, hn_beta, p_ms, p_lambdas and the log marginal
likelihood, as tests/test_mvn.py holds the engine to its fixtures; hn_alpha is exact.  The fixtures' generator refuses a
case whose reference values are further than 2e-12 from a long-double evaluation of the same formulas.
"""
import ctypes
import json
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import regression_oracle as orc
from conftest import GOLDEN, load_golden, rel_err
from regression_error_cases import ar_error_cases, linreg_error_cases

LINREG_CASES = ["linreg_d8_n1000.npz", "linreg_d64_n20000_f32_batches3.npz", "linreg_d128_n30000_f32.npz",
                "linreg_d200_n5000.npz", "linreg_d255_n4000_f32.npz", "linreg_d5_n1.npz"]
AR_CASES = ["ar_p3_t2000.npz", "ar_p16_t50000.npz", "ar_p64_t30000_zeros.npz", "ar_p4_t5.npz"]
TOL = 1e-10


def use_stand_in(m):
    from fake_regression_engine import cpu_factory
    m._reg_pass_factory = cpu_factory
    return m


def prior_of(g):
    return {k: (np.array(v) if isinstance(v, list) else v) for k, v in json.loads(str(g["prior"])).items()}


def make_linreg(g, fake):
    from bayesml_amd import linearregression as lr
    m = lr.LearnModel(int(g["D"]), **prior_of(g))
    return use_stand_in(m) if fake else m


def make_ar(g, fake):
    from bayesml_amd import autoregressive as ar
    m = ar.LearnModel(int(g["p"]), **prior_of(g))
    return use_stand_in(m) if fake else m


def check_linreg(g, m, tol):
    x, y = orc.linreg_inputs(g)
    batches = int(g["batches"])
    for i, (xp, yp) in enumerate(zip(np.array_split(x, batches), np.array_split(y, batches))):
        assert m.update_posterior(xp, yp) is m
        assert rel_err(m.hn_lambda_mat, g[f"b{i}_hn_lambda_mat"]) < tol
        assert rel_err(m.hn_mu_vec, g[f"b{i}_hn_mu_vec"]) < tol
        assert m.hn_alpha == float(g[f"b{i}_hn_alpha"])
        assert rel_err(m.hn_beta, g[f"b{i}_hn_beta"]) < tol
    assert list(m.get_hn_params()) == ["hn_mu_vec", "hn_lambda_mat", "hn_alpha", "hn_beta"]
    assert list(m.get_h0_params()) == ["h0_mu_vec", "h0_lambda_mat", "h0_alpha", "h0_beta"]
    theta, tau = m.estimate_params("squared")
    assert rel_err(theta, g["est_theta"]) < tol and rel_err(tau, g["est_sq_tau"]) < tol
    assert rel_err(m.estimate_params("0-1")[1], g["est_01_tau"]) < tol
    assert rel_err(m.estimate_params("abs")[1], g["est_abs_tau"]) < tol
    assert list(m.estimate_params("squared", dict_out=True)) == ["theta_vec", "tau"]
    t_dist, gamma_dist = m.estimate_params("KL")
    assert t_dist.df == 2.0 * m.hn_alpha and rel_err(gamma_dist.mean(), g["est_sq_tau"]) < tol
    assert rel_err(m.calc_log_marginal_likelihood(), g["lml"]) < tol
    rows = x[:len(g["p_ms"])]
    assert m.calc_pred_dist(rows) is m
    p = m.get_p_params()
    assert list(p) == ["p_ms", "p_lambdas", "p_nus"]
    assert all(type(v) is np.ndarray and v.dtype == np.float64 and v.shape == g["p_ms"].shape for v in p.values())
    assert rel_err(p["p_ms"], g["p_ms"]) < tol and rel_err(p["p_lambdas"], g["p_lambdas"]) < tol
    assert np.array_equal(p["p_nus"], g["p_nus"])
    assert rel_err(m.calc_pred_var(), g["pred_var"]) < tol
    assert rel_err(m.predict(rows), g["p_ms"]) < tol
    assert m.make_prediction("KL").kwds["df"] is m.p_nus
    preds = [m.pred_and_update(g["next_x"][0], float(g["next_y"][0])).copy(),
             m.pred_and_update(g["next_x"][1], float(g["next_y"][1]), loss="0-1").copy()]
    assert rel_err(np.array(preds), g["preds"]) < tol
    assert rel_err(m.hn_mu_vec, g["after_hn_mu_vec"]) < tol and rel_err(m.hn_beta, g["after_hn_beta"]) < tol
    assert m.hn_alpha == float(g["after_hn_alpha"])


def check_ar(g, make, tol):
    x, p, T = g["x"], int(g["p"]), int(g["T"])
    for padding in json.loads(str(g["paddings"])):
        tag = "zeros_" if padding == "zeros" else "none_"
        m = make()
        assert m.update_posterior(x, padding=padding) is m
        assert rel_err(m.hn_lambda_mat, g[tag + "hn_lambda_mat"]) < tol
        assert rel_err(m.hn_mu_vec, g[tag + "hn_mu_vec"]) < tol
        assert m.hn_alpha == float(g[tag + "hn_alpha"])
        assert rel_err(m.hn_beta, g[tag + "hn_beta"]) < tol
        theta, tau = m.estimate_params("squared")
        assert rel_err(theta, g[tag + "est_theta"]) < tol and rel_err(tau, g[tag + "est_sq_tau"]) < tol
        assert rel_err(m.estimate_params("0-1")[1], g[tag + "est_01_tau"]) < tol
        assert rel_err(m.estimate_params("abs")[1], g[tag + "est_abs_tau"]) < tol
        m.calc_pred_dist(x[T - p:])
        assert list(m.get_p_params()) == ["p_m", "p_lambda", "p_nu"]
        assert rel_err(m.p_m, g[tag + "p_m"]) < tol and rel_err(m.p_lambda, g[tag + "p_lambda"]) < tol
        assert m.p_nu == float(g[tag + "p_nu"])
        assert rel_err(np.array(m.predict_interval(0.9)), g[tag + "interval"]) < tol
        assert m.make_prediction("KL").kwds["df"] == m.p_nu
        if tag + "preds" in g:
            m2 = make()
            m2.update_posterior(x[:T - 2], padding=padding)
            preds = [m2.pred_and_update(x[T - 2 - p:T - 1]), m2.pred_and_update(x[T - 1 - p:T], loss="abs")]
            assert rel_err(np.array(preds), g[tag + "preds"]) < tol
            assert rel_err(m2.hn_mu_vec, g[tag + "after_hn_mu_vec"]) < tol
            assert rel_err(m2.hn_beta, g[tag + "after_hn_beta"]) < tol


# ---- the NumPy restatement, pinned to the fixtures at rounding level ----------------------------------------------------
def _h0(D, prior):
    return (np.array(prior.get("h0_mu_vec", np.zeros(D)), dtype=float), np.array(prior.get("h0_lambda_mat", np.eye(D)), dtype=float),
            float(prior.get("h0_alpha", 1.0)), float(prior.get("h0_beta", 1.0)))


@pytest.mark.parametrize("name", LINREG_CASES)
def test_oracle_matches_reference_linreg(name):
    g = load_golden(name)
    D, batches = int(g["D"]), int(g["batches"])
    x, y = orc.linreg_inputs(g)
    mu, lam, alpha, beta = _h0(D, prior_of(g))
    lam0, alpha0, beta0 = lam, alpha, beta
    for i, (xp, yp) in enumerate(zip(np.array_split(x, batches), np.array_split(y, batches))):
        mu, lam, alpha, beta = orc.update(mu, lam, alpha, beta, xp, yp)
        assert rel_err(lam, g[f"b{i}_hn_lambda_mat"]) < 1e-13 and rel_err(mu, g[f"b{i}_hn_mu_vec"]) < 1e-12
        assert alpha == float(g[f"b{i}_hn_alpha"]) and rel_err(beta, g[f"b{i}_hn_beta"]) < 1e-11
    pm, pl, pn = orc.pred_params(mu, lam, alpha, beta, x[:len(g["p_ms"])])
    assert rel_err(pm, g["p_ms"]) < 1e-12 and rel_err(pl, g["p_lambdas"]) < 1e-11 and np.array_equal(pn, g["p_nus"])
    assert rel_err(orc.log_marginal_likelihood(lam0, alpha0, beta0, lam, alpha, beta, int(g["N"])), g["lml"]) < 1e-11


@pytest.mark.parametrize("name", AR_CASES)
def test_oracle_matches_reference_ar(name):
    g = load_golden(name)
    p, T = int(g["p"]), int(g["T"])
    for padding in json.loads(str(g["paddings"])):
        tag = "zeros_" if padding == "zeros" else "none_"
        w, y = orc.lag_matrix(g["x"], p, padding)
        mu, lam, alpha, beta = orc.update(*_h0(p + 1, prior_of(g)), w, y)
        assert rel_err(lam, g[tag + "hn_lambda_mat"]) < 1e-13 and rel_err(mu, g[tag + "hn_mu_vec"]) < 1e-11
        assert alpha == float(g[tag + "hn_alpha"]) and rel_err(beta, g[tag + "hn_beta"]) < 1e-12
        pm, pl, _pn = orc.pred_params(mu, lam, alpha, beta, np.concatenate([[1.0], g["x"][T - p:]])[None, :])
        assert rel_err(pm[0], g[tag + "p_m"]) < 1e-11 and rel_err(pl[0], g[tag + "p_lambda"]) < 1e-12


# ---- host logic through the CPU stand-in ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LINREG_CASES)
def test_linreg_host_logic_with_cpu_stand_in(name):
    g = load_golden(name)
    check_linreg(g, make_linreg(g, fake=True), TOL)


@pytest.mark.parametrize("name", AR_CASES)
def test_ar_host_logic_with_cpu_stand_in(name):
    g = load_golden(name)
    check_ar(g, lambda: make_ar(g, fake=True), TOL)


def _replay(cases, expected_file):
    with open(os.path.join(GOLDEN, expected_file)) as f:
        expected = json.load(f)
    assert set(cases) == set(expected)
    for name, fn in cases.items():
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fn()
            got = None
        except Exception as e:      # noqa: BLE001
            got = type(e).__name__
        assert got == expected[name], name


def test_linreg_boundary_errors_match_reference():
    from bayesml_amd import linearregression as lr
    _replay(linreg_error_cases(lr, use_stand_in), "linreg_errors.json")


def test_ar_boundary_errors_match_reference():
    from bayesml_amd import autoregressive as ar
    _replay(ar_error_cases(ar, use_stand_in), "ar_errors.json")


def test_torch_inputs_and_lazy_predictive_arrays():
    """Torch tensors are accepted like ndarrays (f32 stays f32 on its way to the pass), and p_ms / p_lambdas are fetched
    from the pass's tensors on first read."""
    from bayesml_amd._exceptions import DataFormatError
    g = load_golden("linreg_d8_n1000.npz")
    a = make_linreg(g, fake=True).update_posterior(g["x"], g["y"])
    b = make_linreg(g, fake=True).update_posterior(torch.from_numpy(g["x"]), torch.from_numpy(g["y"]))
    assert np.array_equal(a.hn_mu_vec, b.hn_mu_vec) and a.hn_beta == b.hn_beta
    b.calc_pred_dist(torch.from_numpy(g["x"][:7]))
    assert isinstance(b._p[0], torch.Tensor)
    assert type(b.p_ms) is np.ndarray and b.p_ms.shape == (7,) and not isinstance(b._p[0], torch.Tensor)
    with pytest.raises(DataFormatError):
        b.update_posterior(torch.from_numpy(g["x"]), torch.from_numpy(g["y"][:5]))
    c = make_linreg(g, fake=True)
    assert np.array_equal(c.p_ms, [0.0]) and np.array_equal(c.p_lambdas, [1.0]) and np.array_equal(c.p_nus, [2.0])


def _mixed_dtype_case():
    """f32 regressors (constant last column) with f64 targets around 10: rounding y to f32 moves each by up to 5e-7,
    while c = y.y / (2 hn_beta) stays near 100, so the reference's own formula keeps 13 digits."""
    rng = np.random.default_rng(42)
    x = rng.standard_normal((3000, 12)).astype(np.float32)
    x[:, -1] = 1.0
    theta = rng.standard_normal(12)
    theta[-1] = 10.0
    y = x.astype(np.float64) @ theta + rng.standard_normal(3000)
    assert not np.array_equal(y, y.astype(np.float32).astype(np.float64))
    return x, y


def check_mixed_dtypes(make):
    """update_posterior(x_f32, y_f64) uses y's float64 values: the posterior equals the NumPy update on the widened x
    and the untouched y at 1e-10, and is far (> 1e-9 in hn_beta) from the one a y rounded to f32 gives.  The same the other
    way round (f64 regressors, f32 targets), and for pred_and_update with a Python float."""
    x, y = _mixed_dtype_case()
    D = x.shape[1]
    m = make(D).update_posterior(x, y)
    mu, lam, alpha, beta = orc.update(np.zeros(D), np.eye(D), 1.0, 1.0, x, y)
    assert rel_err(m.hn_mu_vec, mu) < TOL and rel_err(m.hn_lambda_mat, lam) < TOL and rel_err(m.hn_beta, beta) < TOL
    _mu, _lam, _alpha, beta_narrow = orc.update(np.zeros(D), np.eye(D), 1.0, 1.0, x, y.astype(np.float32))
    assert abs(beta_narrow - beta) / beta > 1e-9          # what the test would miss if y were narrowed
    m2 = make(D).update_posterior(torch.from_numpy(x), torch.from_numpy(y))
    assert rel_err(m2.hn_beta, beta) < TOL and rel_err(m2.hn_mu_vec, mu) < TOL
    x64, y32 = x.astype(np.float64) * (1.0 + 2.0 ** -30), y.astype(np.float32)
    m3 = make(D).update_posterior(x64, y32)
    mu3, lam3, _a, beta3 = orc.update(np.zeros(D), np.eye(D), 1.0, 1.0, x64, y32)
    assert rel_err(m3.hn_lambda_mat, lam3) < TOL and rel_err(m3.hn_mu_vec, mu3) < TOL and rel_err(m3.hn_beta, beta3) < TOL
    y_next = 10.0 + 1.0 / 3.0
    m.pred_and_update(x[0], y_next)
    mu4, _l, _a, beta4 = orc.update(mu, lam, alpha, beta, x[:1], np.array([y_next]))
    assert rel_err(m.hn_mu_vec, mu4) < TOL and rel_err(m.hn_beta, beta4) < TOL
    return m


def test_mixed_dtypes_are_not_narrowed_with_cpu_stand_in():
    from bayesml_amd import linearregression as lr
    from bayesml_amd._regression import REGVB_F32, REGVB_F64
    seen = []

    def make(D):
        m = use_stand_in(lr.LearnModel(D))
        factory = m._reg_pass_factory

        def recording(d):
            seen.append(factory(d))
            return seen[-1]
        m._reg_pass_factory = recording
        return m

    check_mixed_dtypes(make)
    # the pass saw each argument in the caller's dtype
    assert seen[0].last_dtypes == (REGVB_F32, REGVB_F64)
    assert any(e.last_dtypes == (REGVB_F64, REGVB_F32) for e in seen)


def test_update_on_zero_rows_is_a_no_op():
    from bayesml_amd import linearregression as lr
    m = lr.LearnModel(3)                                   # (no stand-in: nothing may reach the engine)
    m.update_posterior(np.zeros((0, 3)), np.zeros(0))
    assert m.hn_alpha == 1.0 and m.hn_beta == 1.0 and m._n == 0 and np.array_equal(m.hn_lambda_mat, np.eye(3))


def test_gen_model_streams_match_reference():
    """gen_params / gen_sample consume the Generator like the reference: the fixtures' data came from the reference's
    GenModel with the same seed."""
    from bayesml_amd import autoregressive as ar
    from bayesml_amd import linearregression as lr
    g = load_golden("linreg_d8_n1000.npz")
    gen = lr.GenModel(8, seed=int(g["gen_seed"]))
    gen.gen_params()
    assert np.allclose(gen.theta_vec, g["theta_vec"], rtol=1e-12) and np.isclose(gen.tau, float(g["gen_tau"]), rtol=1e-12)
    x, y = gen.gen_sample(1000)
    assert np.allclose(x, g["x"], rtol=1e-12, atol=1e-14) and np.allclose(y, g["y"], rtol=1e-12, atol=1e-14)
    assert np.all(x[:, -1] == 1.0)
    x2, y2 = lr.GenModel(8, seed=3).gen_sample(x=np.ones((2, 3, 8)))
    assert x2.shape == (6, 8) and y2.shape == (6,)
    g = load_golden("ar_p3_t2000.npz")
    gen = ar.GenModel(3, theta_vec=g["gen_theta_vec"], tau=float(g["gen_tau"]), seed=int(g["gen_seed"]))
    assert np.allclose(gen.gen_sample(2000), g["x"], rtol=1e-12, atol=1e-14)
    assert list(gen.get_h_params()) == ["h_mu_vec", "h_lambda_mat", "h_alpha", "h_beta"]
    assert list(gen.get_params()) == ["theta_vec", "tau"]


def test_pickle_round_trips(tmp_path):
    """h0 / hn dicts survive the positional pickle round trip of base.py, and a fitted model pickles whole."""
    g = load_golden("linreg_d8_n1000.npz")
    m = make_linreg(g, fake=True).update_posterior(g["x"], g["y"])
    f = str(tmp_path / "hn.pkl")
    m.save_hn_params(f)
    m2 = make_linreg(g, fake=True).load_hn_params(f)
    assert np.array_equal(m2.hn_lambda_mat, m.hn_lambda_mat) and m2.hn_beta == m.hn_beta and m2.hn_alpha == m.hn_alpha
    m2.overwrite_h0_params()
    assert np.array_equal(m2.h0_mu_vec, m.hn_mu_vec) and m2.h0_beta == m.hn_beta
    m._reg_pass_factory = None
    m3 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m3.hn_mu_vec, m.hn_mu_vec) and m3._n == 1000 and np.array_equal(m3.p_lambdas, m.p_lambdas)
    g = load_golden("ar_p3_t2000.npz")
    a = make_ar(g, fake=True).update_posterior(g["x"])
    a.save_h0_params(f)
    a.save_hn_params(f)
    a2 = make_ar(g, fake=True).load_hn_params(f)
    assert np.array_equal(a2.hn_mu_vec, a.hn_mu_vec) and a2.hn_beta == a.hn_beta
    a._reg_pass_factory = None
    a3 = pickle.loads(pickle.dumps(a))
    assert np.array_equal(a3.hn_lambda_mat, a.hn_lambda_mat)


def test_plotting_is_out_of_scope(capsys):
    from bayesml_amd import autoregressive as ar
    from bayesml_amd import linearregression as lr
    from bayesml_amd._exceptions import ParameterFormatError
    with pytest.raises(NotImplementedError):
        lr.GenModel(2).visualize_model()
    assert "theta_vec" in capsys.readouterr().out
    with pytest.raises(ParameterFormatError):
        lr.GenModel(3).visualize_model()
    with pytest.raises(NotImplementedError):
        lr.LearnModel(2).visualize_posterior()
    with pytest.raises(ParameterFormatError):
        lr.LearnModel(3).visualize_posterior()
    with pytest.raises(NotImplementedError):
        ar.GenModel(2).visualize_model()
    assert "tau" in capsys.readouterr().out
    with pytest.raises(NotImplementedError):
        ar.LearnModel(1).visualize_posterior()
    with pytest.raises(ParameterFormatError):
        ar.LearnModel(2).visualize_posterior()


def test_engine_limit_at_construction():
    from bayesml_amd import autoregressive as ar
    from bayesml_amd import linearregression as lr
    from bayesml_amd._engine import EngineLimitError
    lr.LearnModel(256)
    ar.LearnModel(255)
    with pytest.raises(EngineLimitError):
        lr.LearnModel(257)
    with pytest.raises(EngineLimitError):
        ar.LearnModel(256)


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bayesml_amd import autoregressive as ar
    from bayesml_amd import linearregression as lr
    from bayesml_amd._engine import EngineUnavailableError
    with pytest.raises(EngineUnavailableError):
        lr.LearnModel(2).update_posterior(np.zeros((4, 2)), np.zeros(4))
    with pytest.raises(EngineUnavailableError):
        lr.LearnModel(2).calc_pred_dist(np.zeros((4, 2)))
    with pytest.raises(EngineUnavailableError):
        ar.LearnModel(2).update_posterior(np.zeros(8))


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------
def test_regvb_argument_errors_without_a_gpu():
    """Pure argument validation returns error codes before anything touches a device."""
    from bayesml_amd import _regression
    lib = _regression.load_library()
    p = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused on its arguments
    F32, EINVAL, EUNSUPPORTED = 0, 1, 2
    assert lib.regvb_stats(0, F32, p, 4, F32, p, 10, p, p, None) == EINVAL
    assert lib.regvb_stats(257, F32, p, 257, F32, p, 10, p, p, None) == EUNSUPPORTED
    assert b"256" in lib.regvb_last_error()
    assert lib.regvb_stats(4, 7, p, 4, F32, p, 10, p, p, None) == EINVAL
    assert b"x_dtype" in lib.regvb_last_error()
    assert lib.regvb_stats(4, F32, p, 4, 2, p, 10, p, p, None) == EINVAL
    assert b"y_dtype" in lib.regvb_last_error()
    assert lib.regvb_stats(4, F32, p, 4, F32, p, 0, p, p, None) == EINVAL
    assert lib.regvb_stats(4, F32, p, 3, 1, p, 10, p, p, None) == EINVAL
    assert b"ldx" in lib.regvb_last_error()
    assert lib.regvb_stats(4, F32, None, 4, F32, p, 10, p, p, None) == EINVAL
    assert lib.regvb_stats(4, F32, p, 4, F32, p, 10, p, None, None) == EINVAL
    assert lib.regvb_stats_window(-1, F32, p, 10, 0, p, p, None) == EINVAL
    assert lib.regvb_stats_window(256, F32, p, 1000, 0, p, p, None) == EUNSUPPORTED
    assert lib.regvb_stats_window(3, F32, p, 3, 0, p, p, None) == EINVAL
    assert b"length" in lib.regvb_last_error()
    assert lib.regvb_stats_window(3, F32, p, 10, 2, p, p, None) == EINVAL
    assert b"padding" in lib.regvb_last_error()
    assert lib.regvb_stats_window(3, F32, None, 10, 0, p, p, None) == EINVAL
    assert lib.regvb_predict(4, F32, p, 4, 10, p, p, 0.0, p, p, p, None) == EINVAL
    assert b"scale" in lib.regvb_last_error()
    assert lib.regvb_predict(300, F32, p, 300, 10, p, p, 1.0, p, p, p, None) == EUNSUPPORTED
    assert lib.regvb_predict(4, F32, p, 4, 0, p, p, 1.0, p, p, p, None) == EINVAL
    assert lib.regvb_predict(4, F32, p, 4, 10, None, p, 1.0, p, p, p, None) == EINVAL


# ---- the real engine -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", LINREG_CASES)
def test_gpu_linreg_matches_reference(name):
    g = load_golden(name)
    m = make_linreg(g, fake=False)
    check_linreg(g, m, TOL)
    assert m._engine.launch_info.startswith("regvb_")


@pytest.mark.gpu
def test_gpu_mixed_dtypes_are_not_narrowed():
    from bayesml_amd import linearregression as lr
    m = check_mixed_dtypes(lambda D: lr.LearnModel(D, device=torch.device("cuda", 0)))
    assert m._engine.launch_info == "regvb_stats"


@pytest.mark.gpu
@pytest.mark.parametrize("name", AR_CASES)
def test_gpu_ar_matches_reference(name):
    g = load_golden(name)
    made = []

    def make():
        made.append(make_ar(g, fake=False))
        return made[-1]

    check_ar(g, make, TOL)
    assert all(m._engine.launch_info == "regvb_stats_window" for m in made)
