"""The five scalar conjugate models (bernoulli, categorical, poisson, exponential, normal) without a GPU: the host logic
through the stand-in engine of tests/fake_expfam_engine.py against the reference's fixtures, the recorded error table, the
GenModel streams, and the argument checks of include/expfam.h."""
import ctypes
import json
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import torch

import expfam_oracle as orc
from conftest import GOLDEN, load_golden
from fake_expfam_engine import CpuExpfamPass, use_cpu

from bayesml_amd import _expfam as xf
from bayesml_amd import bernoulli, categorical, exponential, normal, poisson
from bayesml_amd._engine import EngineLimitError, EngineUnavailableError
from bayesml_amd._exceptions import DataFormatError

MODS = {"bernoulli": bernoulli, "categorical": categorical, "poisson": poisson, "exponential": exponential, "normal": normal}


@pytest.mark.parametrize("name", sorted(orc.CASES))
def test_fixture_through_the_stand_in_engine(name):
    fx = load_golden(name + ".npz")
    got = orc.drive(MODS[orc.CASES[name][0]], name, orc.batches(name, fx), prepare=use_cpu)
    orc.compare(name, got, fx)


@pytest.mark.parametrize("name", sorted(n for n in orc.CASES if orc.CASES[n][4] is None))
def test_gen_model_draws_the_reference_stream(name):
    fx = load_golden(name + ".npz")
    for mine, ref in zip(orc.gen_batches(MODS[orc.CASES[name][0]], name), (fx["x0"], fx["x1"])):
        assert mine.dtype == ref.dtype and np.array_equal(mine, ref)


def test_gen_params_draw_the_reference_stream():
    """gen_params uses the reference's Generator calls in the reference's order (same seed, same parameters)."""
    rng = np.random.default_rng(3)
    assert bernoulli.GenModel(h_alpha=2.0, h_beta=3.0, seed=3).gen_params().theta == rng.beta(2.0, 3.0)
    rng = np.random.default_rng(3)
    assert np.array_equal(categorical.GenModel(4, seed=3).gen_params().theta_vec, rng.dirichlet(np.ones(4) / 2.0))
    rng = np.random.default_rng(3)
    assert poisson.GenModel(h_alpha=2.0, h_beta=4.0, seed=3).gen_params().lambda_ == rng.gamma(shape=2.0, scale=0.25)
    rng = np.random.default_rng(3)
    assert exponential.GenModel(h_alpha=2.0, h_beta=4.0, seed=3).gen_params().lambda_ == rng.gamma(2.0, 0.25)
    rng = np.random.default_rng(3)
    g = normal.GenModel(h_m=1.0, h_kappa=2.0, h_alpha=3.0, h_beta=4.0, seed=3).gen_params()
    tau = rng.gamma(shape=3.0, scale=0.25)
    assert g.tau == tau and g.mu == rng.normal(loc=1.0, scale=1.0 / np.sqrt(tau * 2.0))
    assert list(g.get_h_params()) == ["h_m", "h_kappa", "h_alpha", "h_beta"] and list(g.get_params()) == ["mu", "tau"]


def test_error_table():
    with open(os.path.join(GOLDEN, "expfam_errors.json")) as f:
        recorded = json.load(f)
    cases = orc.error_cases(MODS, prepare=use_cpu)
    assert sorted(cases) == sorted(recorded)
    for name, fn in cases.items():
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fn()
            got = None
        except Exception as e:      # noqa: BLE001
            got = type(e).__name__
        assert got == recorded[name], (name, got, recorded[name])


def _models():
    return [use_cpu(bernoulli.LearnModel(1.5, 2.5)), use_cpu(categorical.LearnModel(3, np.array([1.0, 2.0, 3.0]))),
            use_cpu(poisson.LearnModel(1.5, 2.5)), use_cpu(exponential.LearnModel(1.5, 2.5)),
            use_cpu(normal.LearnModel(0.5, 1.5, 2.5, 3.5))]


GOOD = [np.array([0, 1, 1, 0, 1]), np.array([[0, 0, 1], [1, 0, 0]]), np.array([3, 0, 7]), np.array([0.5, 2.0]),
        np.array([0.5, -2.0, 4.0])]
BAD = [np.array([0, 1, 2]), np.array([[0, 0, 1], [1, 1, 0]]), np.array([3, -1]), np.array([0.5, 0.0]), None]


def _same(a, b):
    return list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_refused_sample_leaves_hn_untouched():
    for m, good, bad in zip(_models(), GOOD, BAD):
        m.update_posterior(good)
        before = {k: np.copy(v) for k, v in m.get_hn_params().items()}
        if bad is not None:
            with pytest.raises(DataFormatError):
                m.update_posterior(bad)
            assert _same(before, m.get_hn_params())


def test_fit_is_reset_then_update():
    for m, good in zip(_models(), GOOD):
        m.update_posterior(good)
        m.update_posterior(good)
        a = type(m)(*m.get_constants().values(), *m.get_h0_params().values())
        use_cpu(a).update_posterior(good)
        assert m.fit(good) is m and _same(m.get_hn_params(), a.get_hn_params())
        assert _same(m.calc_pred_dist().get_p_params(), a.calc_pred_dist().get_p_params())


def test_set_hn_params_clears_the_bookkeeping():
    p = use_cpu(poisson.LearnModel())
    p.update_posterior(np.array([5, 6]))
    assert p._sum_log_factorial > 0
    p.set_hn_params(2.0, 3.0)
    assert p._sum_log_factorial == 0.0
    n = use_cpu(normal.LearnModel())
    n.update_posterior(np.array([5.0, 6.0]))
    n.update_posterior(2.0)
    assert n._n == 3
    n.reset_hn_params()
    assert n._n == 0


def test_pickle_and_save_load_round_trips(tmp_path):
    for m, good in zip(_models(), GOOD):
        m.update_posterior(good)
        m._engine = object()                      # an engine never travels with the model
        c = pickle.loads(pickle.dumps(m))
        assert c._engine is None and _same(c.get_hn_params(), m.get_hn_params()) and _same(c.get_h0_params(), m.get_h0_params())
        f = str(tmp_path / "hn.pkl")
        m.save_hn_params(f)
        d = type(m)(*m.get_constants().values())
        assert _same(d.load_hn_params(f).get_hn_params(), m.get_hn_params())
        m.save_h0_params(f)
        assert _same(d.load_h0_params(f).get_h0_params(), m.get_h0_params())
        assert _same(m.overwrite_h0_params().get_h0_params(),
                     {k.replace("hn_", "h0_"): v for k, v in m.get_hn_params().items()})
    g = normal.GenModel(seed=1)
    f = str(tmp_path / "h.pkl")
    g.save_h_params(f)
    g.save_params(str(tmp_path / "p.pkl"))
    assert _same(normal.GenModel().load_h_params(f).get_h_params(), g.get_h_params())
    g.save_sample(str(tmp_path / "s"), 7)
    assert np.load(str(tmp_path / "s.npz"))["x"].shape == (7,)


def test_scalar_path_needs_no_engine():
    """pred_and_update and scalar updates are host work: no factory, no GPU, no error."""
    def boom():
        raise AssertionError("the engine was asked for")
    for m, item in zip(_models(), [1, np.array([0, 1, 0]), 4, 0.5, -1.25]):
        m._expfam_pass_factory = boom
        m.pred_and_update(item)
        if not isinstance(item, np.ndarray):
            m.update_posterior(item)
            m._update_posterior(item)
    c = categorical.LearnModel(3)
    c._expfam_pass_factory = boom
    c.pred_and_update(2, onehot=False)
    c._update_posterior(1)
    assert np.array_equal(c.hn_alpha_vec, [0.5, 1.5, 1.5])


def test_update_without_check_ignores_bad_values():
    b = use_cpu(bernoulli.LearnModel())._update_posterior(np.array([0, 1, 2, 1]))
    assert (b.hn_alpha, b.hn_beta) == (2.5, 1.5)
    c = use_cpu(categorical.LearnModel(3))._update_posterior(np.array([0, 3, -1, 2, 2]))
    assert np.array_equal(c.hn_alpha_vec, [1.5, 0.5, 2.5])


def test_dtype_plumbing_widens_and_never_narrows():
    eng = CpuExpfamPass()
    for src, kind, want in [(np.int8, "i", torch.int64), (np.int16, "i", torch.int64), (np.uint8, "i", torch.uint8),
                            (np.int32, "i", torch.int32), (np.int64, "i", torch.int64), (np.uint16, "i", torch.int64),
                            (np.uint32, "i", torch.int64), (np.float16, "f", torch.float32), (np.float32, "f", torch.float32),
                            (np.float64, "f", torch.float64), (np.int32, "f", torch.float64)]:
        assert eng.adopt(np.ones((2, 3), dtype=src), kind).dtype == want
        assert eng.adopt(np.ones((2, 3), dtype=src), kind).shape == (6,)
    assert eng.adopt(torch.ones(4, dtype=torch.bfloat16), "f").dtype == torch.float32
    t = torch.arange(24, dtype=torch.int32).reshape(4, 6)
    v = eng.adopt(t[:, :3], "i", cols=3)                      # a strided row matrix is used in place
    assert v.data_ptr() == t.data_ptr() and v.stride(0) == 6
    w = eng.adopt(t[1:], "i")                                 # a view at an element offset is used in place
    assert w.data_ptr() == t[1:].data_ptr() and w.shape == (18,)
    m = use_cpu(normal.LearnModel())
    m.update_posterior(torch.tensor([1.0, 2.0, 4.0], dtype=torch.float32))
    m2 = use_cpu(normal.LearnModel()).update_posterior(np.array([1.0, 2.0, 4.0]))
    assert m.get_hn_params() == m2.get_hn_params()
    with pytest.raises(DataFormatError):
        use_cpu(poisson.LearnModel()).update_posterior(torch.tensor([1.0, 2.0]))
    with pytest.raises(DataFormatError):
        use_cpu(bernoulli.LearnModel()).update_posterior(torch.tensor([True, False]))
    use_cpu(categorical.LearnModel(3)).update_posterior(torch.tensor([[0, 1, 0], [1, 0, 0]], dtype=torch.uint8))


def test_degree_limit_is_reported_at_construction():
    categorical.LearnModel(xf.MAX_DEGREE)
    with pytest.raises(EngineLimitError):
        categorical.LearnModel(xf.MAX_DEGREE + 1)


def test_visualize_prints_then_refuses(capsys):
    with pytest.raises(NotImplementedError):
        bernoulli.GenModel().visualize_model()
    assert capsys.readouterr().out == "theta:0.5\n"
    with pytest.raises(NotImplementedError):
        categorical.GenModel(3).visualize_model()
    assert capsys.readouterr().out.startswith("theta_vec:[0.33333333")
    with pytest.raises(NotImplementedError):
        poisson.GenModel(seed=0).visualize_model(5)
    assert re.fullmatch(r"lambda:1.0\nx:\[\d \d \d \d \d\]\n", capsys.readouterr().out)
    with pytest.raises(NotImplementedError):
        exponential.GenModel().visualize_model()
    assert capsys.readouterr().out == "lambda_:1.0\n"
    with pytest.raises(NotImplementedError):
        normal.GenModel().visualize_model()
    with pytest.raises(NotImplementedError):
        categorical.LearnModel(3).visualize_posterior()
    assert capsys.readouterr().out == "hn_alpha_vec:[0.5 0.5 0.5]\n"
    for m in (bernoulli.LearnModel(), poisson.LearnModel(), exponential.LearnModel(), normal.LearnModel()):
        with pytest.raises(NotImplementedError):
            m.visualize_posterior()


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------
def test_block_and_scratch_lengths():
    lib = xf.load_library()
    want = {xf.BERNOULLI: 4, xf.COUNTS: 3 + 17, xf.ONEHOT: 2 + 17, xf.POISSON: 4, xf.EXPONENTIAL: 3, xf.NORMAL: 3}
    for family, n in want.items():
        assert lib.expfam_stats_len(family, 17) == n
        assert lib.expfam_work_len(family, 17) >= 1024 * (n - 1)
    for family in (xf.COUNTS, xf.ONEHOT):
        assert lib.expfam_stats_len(family, 0) == -1 and lib.expfam_stats_len(family, xf.MAX_DEGREE + 1) == -1
        assert lib.expfam_work_len(family, xf.MAX_DEGREE + 1) == -1 and lib.expfam_stats_len(family, xf.MAX_DEGREE) > 0
    assert lib.expfam_stats_len(6, 1) == -1 and lib.expfam_stats_len(-1, 1) == -1 and lib.expfam_stats_len(xf.NORMAL, 0) == 3


def test_argument_errors_without_a_gpu():
    """Every argument is checked before anything touches the device: the pointers below are never dereferenced."""
    lib = xf.load_library()
    p = ctypes.c_void_p(4096)
    EINVAL, EUNSUPPORTED = 1, 2
    assert lib.expfam_stats_counts(xf.I32, p, 10, 0, p, p, None) == EINVAL and b"degree" in lib.expfam_last_error()
    assert lib.expfam_stats_counts(xf.I32, p, 10, xf.MAX_DEGREE + 1, p, p, None) == EUNSUPPORTED
    assert lib.expfam_stats_onehot(xf.U8, p, 10, xf.MAX_DEGREE + 1, xf.MAX_DEGREE + 1, p, p, None) == EUNSUPPORTED
    assert lib.expfam_stats_onehot(xf.U8, p, 10, 0, 4, p, p, None) == EINVAL
    assert lib.expfam_stats_onehot(xf.U8, p, 10, 4, 3, p, p, None) == EINVAL and b"ld" in lib.expfam_last_error()
    one = [lib.expfam_stats_bernoulli, lib.expfam_stats_poisson, lib.expfam_stats_exponential, lib.expfam_stats_normal]
    for fn, good in zip(one, (xf.U8, xf.I64, xf.F32, xf.F64)):
        assert fn(good, p, 0, p, p, None) == EINVAL and b"n must be" in lib.expfam_last_error()
        assert fn(good, p, -5, p, p, None) == EINVAL
        assert fn(5, p, 10, p, p, None) == EINVAL and b"dtype" in lib.expfam_last_error()
        assert fn(-1, p, 10, p, p, None) == EINVAL
        assert fn(good, None, 10, p, p, None) == EINVAL and b"null" in lib.expfam_last_error()
        assert fn(good, p, 10, None, p, None) == EINVAL and fn(good, p, 10, p, None, None) == EINVAL
    for fn in (lib.expfam_stats_bernoulli, lib.expfam_stats_poisson):                 # a float dtype to an integer family
        assert fn(xf.F32, p, 10, p, p, None) == EINVAL and fn(xf.F64, p, 10, p, p, None) == EINVAL
    assert lib.expfam_stats_counts(xf.F64, p, 10, 4, p, p, None) == EINVAL
    assert lib.expfam_stats_onehot(xf.F32, p, 10, 4, 4, p, p, None) == EINVAL
    for fn in (lib.expfam_stats_exponential, lib.expfam_stats_normal):                 # and an integer dtype to a float family
        assert fn(xf.I32, p, 10, p, p, None) == EINVAL
    assert lib.expfam_stats_normal(xf.F64, ctypes.c_void_p(4100), 10, p, p, None) == EINVAL     # not aligned to 8 bytes
    assert b"aligned" in lib.expfam_last_error()


def test_product_path_fails_loudly_without_gpu():
    for m, good in zip([bernoulli.LearnModel(), categorical.LearnModel(3), poisson.LearnModel(), exponential.LearnModel(),
                        normal.LearnModel()], GOOD):
        if torch.cuda.is_available():
            return                              # (an unmarked test does not touch the device)
        with pytest.raises(EngineUnavailableError):
            m.update_posterior(good)
        with pytest.raises(EngineUnavailableError):
            type(m)(*m.get_constants().values(), device="cpu").update_posterior(good)
