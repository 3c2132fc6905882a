"""The HMM sequence predictive on the CPU: the NumPy restatement of the engine (tests/hmmpred_oracle.py) against the exact
oracle inside the derived bound B_t, the two sticky chains on which forgetting fails - with the repair off the restatement
misses the bound behind a boundary, with it on it holds, so the GPU cases can fail -, the C ABI of include/hmmpred.h without
a GPU, and ``hiddenmarkovnormal.LearnModel.calc_pred_logpdf`` through the ``_hmmpred_pass_factory`` seam.

Measured here (worst |error| / B_t of the restatement, no factor): 0.001 (nu_1_and_1e8) to 0.028 (k5_d17_cond1e4) over the
fourteen recipes of tests/hmmpred_cases.py; without the repair the sticky chains miss the bound at 167 of 200 steps, by up
to 2.0e11 times.
"""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import hmmpred_cases as cases
import hmmpred_oracle as ho
from conftest import ROOT

_cache = {}


def recipe(name):
    """(case, plan keywords, exact oracle about the default pivot), made once and shared."""
    if name not in _cache:
        c = cases.RECIPES[name]()
        kw = cases.CHUNK if name in cases.STICKY else {}
        _cache[name] = (c, kw, ho.exact(c["a"], c["w0"], c["u"], c["mu"], c["nu"], c["x"][0], c["x"], **kw))
    return _cache[name]


def args(c):
    return c["x"], c["a"], c["w0"], c["mu"], c["nu"], c["u"]


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.RECIPES)
def test_restatement_is_inside_the_bound(name):
    c, kw, o = recipe(name)
    lnp, z, end, diag = ho.restate(*args(c), **kw)
    worst, at = o.ratio(lnp)
    print(f"{name}: worst |error| / B_t = {worst:.3f} at step {at}; end vector {o.end_ratio(end):.3f} of its bound")
    assert worst <= 1.0
    decided = o.z_decided(1.0)
    assert decided.any() and np.array_equal(z[decided], o.z[decided])
    assert o.end_ratio(end) <= 1.0
    assert abs(float(np.sum(o.phi[-1])) - 1.0) < 1e-12


@pytest.mark.parametrize("name", cases.ORDINARY)
def test_the_bound_cannot_hide_a_failure(name):
    """Every ordinary case keeps B_t below 1e-9 (1 + |ln p_t|); cases.HARD lists the only exemptions by name."""
    _, _, o = recipe(name)
    assert np.all(o.B <= 1e-9 * (1.0 + np.abs(o.lnp))), (name, float(np.max(o.B / (1.0 + np.abs(o.lnp)))))


def test_the_hard_cases_are_the_ones_named():
    assert sorted(cases.HARD) == ["badly_scaled", "far_means", "nu_1_and_1e8"]
    c = cases.HARD["far_means"]()
    assert np.abs(c["mu"]).min() > 9e5
    c = cases.HARD["nu_1_and_1e8"]()
    assert c["nu"].min() == 1.0 and c["nu"].max() == 1e8
    c = cases.HARD["badly_scaled"]()
    assert np.linalg.cond(np.tril(c["u"][0]).T @ np.tril(c["u"][0])) > 1e5


@pytest.mark.parametrize("name", cases.STICKY)
def test_sticky_chains_open_the_gate_and_need_the_repair(name):
    c, kw, o = recipe(name)
    assert np.allclose(np.diag(c["a"]), 1.0 - 1e-3) and np.allclose(np.diff(c["mu"][:, 0]), 0.5)
    parallel, L, W, n_chunks = ho.plan(3, len(c["x"]), **kw)
    assert parallel and (L, W) == (32, 8) and n_chunks == 7
    lnp, z, end, diag = ho.restate(*args(c), **kw)
    assert diag[0] >= 1 and diag[1] >= 1                         # the gate opened, chunks were walked again
    assert o.ratio(lnp)[0] <= 1.0 and o.end_ratio(end) <= 1.0
    off, _, off_end, off_diag = ho.restate(*args(c), **kw, repair=False)
    assert off_diag[1] == 0
    mp = ho.orc._mp()
    err = np.array([float(abs(mp.mpf(float(g)) - e)) for g, e in zip(off, o.lnp_mp)])
    missed = np.flatnonzero(err > o.B)
    print(f"{name}: diag = {diag.tolist()}; without the repair {len(missed)} steps miss the bound, the first at {missed[:1]}, "
          f"worst {float((err / o.B).max()):.3g} bounds")
    assert len(missed) > 0 and missed.min() > L                  # (chunk 0 starts from phi_0 itself)
    assert np.all(err[:L + 1] <= o.B[:L + 1])
    assert {int((t - 1) // L) for t in missed} <= set(range(1, n_chunks))
    if name == "sticky_flat_stretch":
        assert np.all(c["x"][60:70] == 1e4) and 64 in range(60, 70)      # across the boundary behind step 64


def test_a_mixing_chain_stands():
    c = cases.make(3, 2, 200, 21, stay=0.3, sep=8.0)
    lnp, z, end, diag = ho.restate(*args(c), **cases.CHUNK)
    assert diag.tolist() == [0, 0]
    serial, zs, _, _ = ho.restate(*args(c))
    assert np.allclose(lnp, serial, rtol=0, atol=1e-11) and np.array_equal(z, zs)


def test_a_duplicated_state_yields_the_lower_index():
    c = cases.duplicate_state(cases.make(4, 3, 60, 22), 1, 3)
    lnp, z, end, _ = ho.restate(*args(c))
    assert end[1] == end[3] and 3 not in z and 1 in z


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree():
    from bayesml_amd import _hmmpred
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/hmmpred.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hmmpred_[a-z0-9_]+)\s*\(", text)))
    lib = _hmmpred.load_library()
    assert sorted(_hmmpred.SYMBOLS) == declared and len(declared) == 4
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.hmmpred_abi_version() == 1 == int(re.search(r"#define HMMPRED_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MAX_DEGREE", _hmmpred.MAX_DEGREE), ("MAX_STATES", _hmmpred.MAX_STATES),
                         ("PARALLEL_STATES", _hmmpred.PARALLEL_STATES), ("MIN_CHUNK", _hmmpred.MIN_CHUNK)):
        assert int(re.search(rf"#define HMMPRED_{macro} (\d+)", text).group(1)) == value
    assert (_hmmpred.MIN_CHUNK, _hmmpred.PARALLEL_STATES, _hmmpred.FORGET_TOL) == (ho.MIN_CHUNK, ho.PARALLEL_STATES, ho.TOL)


def test_scratch_len_against_its_restatement():
    from bayesml_amd import _hmmpred
    lib = _hmmpred.load_library()
    for K in (1, 16, 17, 64, 65, 256):
        for n in (1, 2, 8, 9, 10, 63, 64, 65, 4096, 10 ** 7):
            got = lib.hmmpred_scratch_len(K, 3, n)
            assert got == _hmmpred.scratch_len(K, 3, n) > 0 and got % 2 == 0
    assert lib.hmmpred_scratch_len(32, 16, 1000) == 2 * 1024 * 32 + 2 * 1024 + 2 * 126 * 32 + 2
    for K, D, n in ((0, 3, 10), (257, 3, 10), (3, 0, 10), (3, 19201, 10), (3, 3, 0)):
        assert lib.hmmpred_scratch_len(K, D, n) == -1
    for K in (3, 40, 200):
        for budget in (1 << 12, 1 << 16, 1 << 20, 1 << 30):
            n = _hmmpred.slice_rows(K, 3, budget)
            assert n >= 1 and (n == 1 or 8 * _hmmpred.scratch_len(K, 3, n) <= budget)
            assert n == 1 or 8 * _hmmpred.scratch_len(K, 3, 2 * n) > budget          # (and not needlessly short)
    for T in (1, 4095, 4096, 32768, 32769):
        L, W = _hmmpred.default_plan(T)
        assert ho.plan(3, T)[1:3] == ((L, W) if L else (T, min(64, T)))


def test_argument_errors_without_a_gpu():
    from bayesml_amd import _hmmpred
    lib = _hmmpred.load_library()
    P, odd, odd16 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)          # never dereferenced

    def call(K=3, D=4, xt=0, x=P, ldx=4, n=10, pivot=P, img=P, c=P, nu=P, a=P, w0=P, chunk=0, sweep=0, scratch=P, lnp=P, z=P,
             end=P, diag=P):
        return lib.hmmpred_logpdf(K, D, xt, x, ldx, n, pivot, img, c, nu, a, w0, chunk, sweep, scratch, lnp, z, end, diag, None)

    def refused(rc, text, code=1):
        assert rc == code and text in lib.hmmpred_last_error().decode(), (rc, lib.hmmpred_last_error())

    refused(call(K=0), "K must be >= 1")
    refused(call(K=257), "at most 256 states", code=2)          # HMMPRED_EUNSUPPORTED
    refused(call(K=65536), "at most 256 states", code=2)
    refused(call(D=0), "D must be in 1..19200")
    refused(call(D=19201, ldx=19201), "D must be in 1..19200")
    refused(call(n=0), "n_rows")
    refused(call(xt=2), "x_dtype")
    refused(call(ldx=3), "ldx")
    refused(call(chunk=7), "chunk_len")
    refused(call(chunk=-1), "chunk_len")
    refused(call(sweep=-1), "sweep_len")
    for null in ("x", "pivot", "img", "c", "nu", "a", "w0", "scratch", "lnp", "end", "diag"):
        refused(call(**{null: None}), "null pointer")
    refused(call(xt=1, x=odd), "aligned to its element size")
    for name in ("pivot", "c", "nu", "a", "w0", "lnp", "z", "end", "diag"):
        refused(call(**{name: odd}), "8-byte aligned")
    refused(call(img=odd16), "16-byte aligned")
    refused(call(scratch=odd16), "16-byte aligned")


# ---- the model on the stand-in ---------------------------------------------------------------------------------------------
def hmm(K=3, D=2, seed=0):
    """A model with a posterior that is not the prior's, set by hand (no data pass on the CPU)."""
    from bayesml_amd import hiddenmarkovnormal as hm
    rng = np.random.default_rng(seed)
    m = hm.LearnModel(K, D, seed=0, verbose=False)
    w = rng.standard_normal((K, D, D))
    m.set_hn_params(hn_eta_vec=rng.uniform(1.0, 5.0, K), hn_zeta_vecs=rng.uniform(0.5, 5.0, (K, K)) + 6.0 * np.eye(K),
                    hn_m_vecs=3.0 * rng.standard_normal((K, D)), hn_kappas=rng.uniform(1.0, 9.0, K),
                    hn_nus=D + rng.uniform(0.0, 20.0, K), hn_w_mats=w @ w.transpose(0, 2, 1) + np.eye(D))
    g = rng.uniform(0.1, 1.0, K)
    m._gamma_last[:] = g / g.sum()
    m._hmmpred_pass_factory = ho.StandIn
    return m


def scipy_filter(m, x, w0):
    """(ln p [T], phi [T, K]) by a float64 NumPy filter over scipy's Student-t densities of ``get_p_params()``."""
    from scipy.special import logsumexp
    from scipy.stats import multivariate_t
    p = m.get_p_params()
    K = m.c_num_classes
    le = np.stack([multivariate_t(loc=p["p_mu_vecs"][k], shape=np.linalg.inv(p["p_lambda_mats"][k]), df=p["p_nus"][k]).logpdf(x)
                   .reshape(-1) for k in range(K)], axis=1)
    w, lnp, phi = np.asarray(w0, dtype=np.float64), np.empty(len(x)), np.empty((len(x), K))
    for t in range(len(x)):
        with np.errstate(divide="ignore"):
            lt = np.log(w) + le[t]
        lnp[t] = logsumexp(lt)
        phi[t] = np.exp(lt - lnp[t])
        w = phi[t] @ p["p_a_mat"]
    return lnp, phi


def test_calc_pred_logpdf_on_the_stand_in():
    from bayesml_amd._exceptions import ParameterFormatError
    K, D, T = 3, 2, 90
    m = hmm(K, D)
    x = 3.0 * np.random.default_rng(5).standard_normal((T, D))
    before = pickle.dumps((m.get_hn_params(), m.hn_w_mats_inv, m._engine, m._gamma_last, m.ns, m.ms, m.x_bar_vecs, m.s_mats))
    m.p_nus[:] = -1.0                                          # stale on purpose: the call refreshes them
    lnp = m.calc_pred_logpdf(x)
    assert isinstance(lnp, np.ndarray) and lnp.dtype == np.float64 and lnp.shape == (T,)
    assert np.array_equal(m.p_nus, m.hn_nus - D + 1)
    # the three kinds of start
    want, phi = scipy_filter(m, x, m._gamma_last @ m.p_a_mat)
    assert np.allclose(lnp, want, rtol=1e-10, atol=1e-10)
    assert np.array_equal(lnp, m.calc_pred_logpdf(x, start="last"))
    fresh = m.calc_pred_logpdf(x, start="initial")
    assert np.allclose(fresh, scipy_filter(m, x, m.hn_eta_vec / m.hn_eta_vec.sum())[0], rtol=1e-10, atol=1e-10)
    assert not np.array_equal(fresh, lnp)
    w0 = np.array([0.0, 0.25, 0.75])
    for given in (w0, list(w0), torch.from_numpy(w0)):
        assert np.allclose(m.calc_pred_logpdf(x, start=given), scipy_filter(m, x, w0)[0], rtol=1e-10, atol=1e-10)
    calls = ho.StandIn.calls
    for bad in ("first", np.array([0.5, 0.5]), np.array([0.5, 0.6, -0.1]), np.array([0.3, 0.3, 0.3]), np.array([np.nan, 0.5, 0.5]),
                np.full((1, 3), 1 / 3), None, 1.0, np.array([0.5, 0.5, 1e-9])):
        with pytest.raises(ParameterFormatError):
            m.calc_pred_logpdf(x, start=bad)
    with pytest.raises(ParameterFormatError):
        m.calc_pred_logpdf(x, chunk_bytes=0)
    assert ho.StandIn.calls == calls
    # return kinds
    l2, z = m.calc_pred_logpdf(x, assign=True)
    clear = np.sort(phi, axis=1)[:, -1] - np.sort(phi, axis=1)[:, -2] > 1e-9
    assert np.array_equal(l2, lnp) and z.dtype == np.int64 and z.shape == (T,) and np.array_equal(z[clear], phi.argmax(axis=1)[clear])
    l3, state = m.calc_pred_logpdf(x, return_state=True)
    assert np.array_equal(l3, lnp) and state.shape == (K,) and np.allclose(state, phi[-1], rtol=1e-9, atol=1e-300)
    l4, z4, s4 = m.calc_pred_logpdf(x, assign=True, return_state=True)
    assert np.array_equal(l4, lnp) and np.array_equal(z4, z) and np.array_equal(s4, state)
    tl, tz, ts = m.calc_pred_logpdf(torch.from_numpy(x), assign=True, return_state=True)
    assert all(isinstance(v, torch.Tensor) for v in (tl, tz, ts)) and tl.dtype == torch.float64 and tz.dtype == torch.int64
    assert np.array_equal(tl.numpy(), lnp) and np.array_equal(tz.numpy(), z) and np.array_equal(ts.numpy(), state)
    # one row, no rows, f32 rows, leading axes
    one = m.calc_pred_logpdf(x[7])
    assert one.shape == (1,) and np.allclose(one, scipy_filter(m, x[7:8], m._gamma_last @ m.p_a_mat)[0], rtol=1e-10)
    e_l, e_z, e_s = m.calc_pred_logpdf(np.zeros((0, D)), assign=True, return_state=True)
    assert e_l.shape == (0,) and e_z.shape == (0,) and e_z.dtype == np.int64 and np.array_equal(e_s, m._gamma_last @ m.p_a_mat)
    l32 = m.calc_pred_logpdf(x.astype(np.float32))
    assert l32.dtype == np.float64 and np.array_equal(l32, m.calc_pred_logpdf(x.astype(np.float32).astype(np.float64)))
    assert m.calc_pred_logpdf(x.reshape(9, 10, D)).shape == (T,)
    # nothing of the fit has changed, and the model pickles (the seam is a class, the model holds no engine of this pass)
    assert pickle.dumps((m.get_hn_params(), m.hn_w_mats_inv, m._engine, m._gamma_last, m.ns, m.ms, m.x_bar_vecs, m.s_mats)) == before
    assert m._engine is None and np.array_equal(pickle.loads(pickle.dumps(m)).calc_pred_logpdf(x), lnp)


def test_slices_and_continuation_on_the_stand_in():
    from bayesml_amd import _hmmpred
    K, D, T = 3, 2, 300
    m = hmm(K, D, seed=1)
    x = 3.0 * np.random.default_rng(6).standard_normal((T, D))
    whole, z, state = m.calc_pred_logpdf(x, assign=True, return_state=True)
    budget = 8 * _hmmpred.scratch_len(K, D, 64)
    step = _hmmpred.slice_rows(K, D, budget)
    assert 3 <= -(-T // step) and step >= 64
    calls = ho.StandIn.calls
    cut, zc, sc = m.calc_pred_logpdf(x, assign=True, return_state=True, chunk_bytes=budget)
    assert ho.StandIn.calls - calls == -(-T // step)
    assert np.allclose(cut, whole, rtol=0, atol=1e-12) and np.array_equal(zc, z) and np.allclose(sc, state, rtol=1e-12)
    # a stream continued across calls
    first, s1 = m.calc_pred_logpdf(x[:130], return_state=True)
    second = m.calc_pred_logpdf(x[130:], start=s1 @ m.p_a_mat)
    assert np.allclose(np.concatenate([first, second]), whole, rtol=0, atol=1e-12)


def test_t1_is_the_weighted_student_t_mixture():
    from scipy.stats import multivariate_t
    m = hmm(4, 3, seed=2)
    x = np.random.default_rng(7).standard_normal(3)
    p = m.get_p_params()
    for start, w0 in (("last", m._gamma_last @ m.p_a_mat), ("initial", m.hn_eta_vec / m.hn_eta_vec.sum())):
        want = np.log(sum(w0[k] * multivariate_t.pdf(x, loc=p["p_mu_vecs"][k], shape=np.linalg.inv(p["p_lambda_mats"][k]),
                                                     df=p["p_nus"][k]) for k in range(4)))
        got = m.calc_pred_logpdf(x, start=start)
        assert got.shape == (1,) and abs(got[0] - want) <= 1e-10 * abs(want)


def test_bad_rows_are_refused_with_the_model_untouched():
    from bayesml_amd._exceptions import DataFormatError
    m = hmm()
    m.p_nus[:] = -1.0
    before = pickle.dumps(m.__dict__)
    calls = ho.StandIn.calls
    for bad in (np.zeros((4, 3)), np.zeros((4, 2), dtype=complex), np.array(1.0), [[0.0, 1.0]], torch.zeros(4, 3),
                torch.zeros(4, 2, dtype=torch.int64)):
        with pytest.raises(DataFormatError) as e:
            m.calc_pred_logpdf(bad)
        with pytest.raises(DataFormatError) as e2:
            m._check_rows(bad)
        assert str(e.value) == str(e2.value)
    assert pickle.dumps(m.__dict__) == before and ho.StandIn.calls == calls


def test_limits_and_no_gpu():
    from bayesml_amd import hiddenmarkovnormal as hm
    from bayesml_amd._engine import EngineLimitError, EngineUnavailableError
    with pytest.raises(EngineLimitError, match="c_num_classes <= 256"):
        hm.LearnModel(257, 1, verbose=False).calc_pred_logpdf(np.zeros((4, 1)))
    if torch.cuda.is_available():
        return                              # (an unmarked test does not touch the device)
    with pytest.raises(EngineUnavailableError):
        hm.LearnModel(3, 2, verbose=False).calc_pred_logpdf(np.zeros((4, 2)))
