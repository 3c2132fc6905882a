"""The HMM sequence predictive on the device (include/hmmpred.h) against the exact oracle of tests/hmmpred_oracle.py: every
ln p_t within 2 B_t of the exact value (B_t: the derived bound there; 2 is its only margin), z_t equal to the oracle's
wherever the two largest phi differ in the log by more than 2 H_t, phi_{T-1} within a relative 2 H_{T-1}, the same bits
from every storage of the same rows and from two calls, nothing written past the end.  chunk_len = 32, sweep_len = 8 unless
stated, so that a few hundred steps cross chunks, waves (16 chunks) and workgroups (64 chunks).  Every test prints its worst
|error| / B_t (profiles/hmmpred.md has them): measured 0.001 to 0.040 over all cases, the largest on the mixing chain; the
model tests 6.6e-13 against their 1e-9 and below.
"""
import numpy as np
import pytest
import torch

import hmmpred_cases as cases
import hmmpred_oracle as ho
import stmix_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = cases.CHUNK
_cache = {}


def engine(K, D):
    from bayesml_amd import _hmmpred
    return _hmmpred.HmmFilterPass(K, D, DEV)


def run(c, x=None, want_z=True, eng=None, w0=None, pivot=None, **kw):
    """(ln p, z, end, diag, engine) as NumPy arrays for the rows ``x`` (default: the case's, float64)."""
    K, D = c["mu"].shape
    eng = eng or engine(K, D)
    xd = eng.adopt(c["x"] if x is None else x)
    lnp, z, end, diag = eng.run(xd, c["a"], c["w0"] if w0 is None else w0, c["mu"], c["nu"], c["u"], want_z, pivot=pivot, **kw)
    torch.cuda.synchronize()
    return lnp.cpu().numpy(), (z.cpu().numpy() if want_z else None), end.cpu().numpy(), diag.cpu().numpy(), eng


def check(label, o, lnp, z, end):
    worst, at = o.ratio(lnp)
    e = o.end_ratio(end, 2.0)
    print(f"{label}: worst |error| / B_t = {worst:.3f} at step {at} of {len(lnp)}; end vector {e:.3f} of its bound")
    assert worst <= 2.0, (label, worst, at)
    if z is not None:
        decided = o.z_decided(2.0)
        assert np.array_equal(z[decided], o.z[decided]), label
        assert z.min() >= 0 and z.max() < o.phi.shape[1]
    assert e <= 1.0, (label, e)


def held(label, c, x=None, **kw):
    """Run, and hold the results to the oracle built from what the engine was handed."""
    lnp, z, end, diag, eng = run(c, x, **kw)
    o = ho.exact_of(eng.last, c["x"] if x is None else x)
    check(label, o, lnp, z, end)
    return lnp, z, end, diag, o


# ---- shape edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 2, 15, 16, 17, 33, 64, 128, 129, 200))
def test_every_feature_tile_count_and_the_plain_path(D):
    held(f"D = {D}", cases.make(5, D, 100, 100 + D), **CHUNK)


@pytest.mark.parametrize("K", (1, 2, 15, 16, 17, 32, 33, 48, 64, 65, 100, 256))
def test_every_state_block_count_and_the_serial_walk(K):
    """Every 16-state block count of the replay, the switch to the serial walk at 65 and its top; A banded from 17 states on
    (the oracle skips the zeros)."""
    from bayesml_amd import _hmmpred
    c = cases.make(K, 3, 100 if K <= 64 else 40, 200 + K, band=None if K <= 17 else 3)
    lnp, z, end, diag, o = held(f"K = {K}", c, **CHUNK)
    assert (K <= _hmmpred.PARALLEL_STATES) == ho.plan(K, len(c["x"]), **CHUNK)[0]


def test_more_than_256_states_are_refused():
    from bayesml_amd import _hmmpred, hiddenmarkovnormal as hm
    from bayesml_amd._engine import EngineLimitError
    with pytest.raises(EngineLimitError):
        engine(257, 3)
    with pytest.raises(EngineLimitError):
        hm.LearnModel(257, 1, verbose=False, device=DEV).calc_pred_logpdf(np.zeros((4, 1)))
    assert _hmmpred.load_library().hmmpred_scratch_len(257, 3, 10) == -1


def long_case():
    if "long" not in _cache:
        c = cases.make(3, 2, 2090, 300)
        _cache["long"] = (c, ho.exact(c["a"], c["w0"], c["u"], c["mu"], c["nu"], c["x"][0], c["x"], **CHUNK))
    return _cache["long"]


@pytest.mark.parametrize("T", (1, 2, 32, 33, 34, 513, 514, 2049, 2050, 2090))
def test_lengths_around_a_chunk_a_wave_and_a_workgroup(T):
    """One chunk ends at step 32, a wave's 16 chunks at 512, a workgroup's 64 at 2048.  The outputs lie inside larger
    buffers of guard values: nothing past entry T - 1 (K - 1 of end, 1 of diag) is written, with z and with z NULL."""
    c, whole = long_case()
    o = whole.prefix(T, **CHUNK)
    eng = engine(3, 2)
    for want_z in (True, False):
        g = dict(lnp=torch.full((T + 64,), -7.0, dtype=torch.float64, device=DEV), z=torch.full((T + 64,), -7, dtype=torch.int64, device=DEV),
                 end=torch.full((3 + 64,), -7.0, dtype=torch.float64, device=DEV), diag=torch.full((2 + 64,), -7, dtype=torch.int64, device=DEV))
        out = dict(lnp=g["lnp"][:T], z=g["z"][:T], end=g["end"][:3], diag=g["diag"][:2])
        lnp, z, end, diag, _ = run(c, c["x"][:T], want_z=want_z, eng=eng, out=out, **CHUNK)
        check(f"T = {T}, z {'wanted' if want_z else 'NULL'}", o, lnp, z, end)
        for key, n in (("lnp", T), ("z", T if want_z else 0), ("end", 3), ("diag", 2)):
            assert bool((g[key][n:] == -7).all()), (key, T, want_z)
        # (sweeps of 8 steps do not always stand on this chain: the repair is part of what the lengths are run through)
        assert 0 <= diag[1] <= max(0, ho.plan(3, T, **CHUNK)[3] - 1) and (diag[0] > 0) == (diag[1] > 0)


def test_default_chunks_across_the_4096_step_switch():
    c = cases.make(3, 2, 5000, 301)
    assert ho.plan(3, 5000)[:3] == (True, 32, 32) and not ho.plan(3, 4095)[0]
    lnp, z, end, diag, o = held("T = 5000, default plan", c)
    assert diag.tolist() == [0, 0]
    short = run(c, c["x"][:4095])
    check("T = 4095, default plan (serial)", o.prefix(4095), *short[:3])


# ---- storage, determinism ------------------------------------------------------------------------------------------------
def test_storage_does_not_change_a_bit():
    D, n = 33, 100
    c = cases.make(4, D, n, 302, f32=True)
    eng = engine(4, D)
    base = run(c, torch.from_numpy(c["x"]).to(DEV), eng=eng, **CHUNK)
    check("D = 33, float64", ho.exact_of(eng.last, c["x"]), *base[:3])
    x32 = torch.from_numpy(c["x"].astype(np.float32)).to(DEV)
    wide = torch.zeros(n, D + 3, dtype=torch.float64, device=DEV)
    wide[:, :D] = torch.from_numpy(c["x"]).to(DEV)
    wide32 = torch.zeros(n, D + 4, dtype=torch.float32, device=DEV)
    wide32[:, :D] = x32
    assert wide[:, :D].stride(0) == D + 3
    for label, xs in (("float32", x32), ("float64 strided", wide[:, :D]), ("float32 strided", wide32[:, :D]),
                      ("NumPy float32", c["x"].astype(np.float32)), ("again", torch.from_numpy(c["x"]).to(DEV))):
        got = run(c, xs, eng=eng, **CHUNK)
        for u, v in zip(got[:4], base[:4]):
            assert np.array_equal(u, v), label


def test_vector_loads_give_the_same_bits():
    D, n = 16, 70
    c = cases.make(3, D, n, 303, f32=True)
    eng = engine(3, D)
    x = torch.from_numpy(c["x"]).to(DEV)
    base = run(c, x, eng=eng, **CHUNK)
    flat = torch.zeros(n * D + 1, dtype=torch.float64, device=DEV)
    flat[1:] = x.reshape(-1)
    got = run(c, flat[1:].view(n, D), eng=eng, **CHUNK)            # (one element in: scalar loads)
    for u, v in zip(got[:4], base[:4]):
        assert np.array_equal(u, v)


# ---- repair and exactness ------------------------------------------------------------------------------------------------
def test_a_mixing_chain_with_separated_emissions_stands():
    c = cases.make(3, 2, 400, 21, stay=0.3, sep=8.0)
    lnp, z, end, diag, o = held("mixing chain", c, **CHUNK)
    assert diag.tolist() == [0, 0]


@pytest.mark.parametrize("name", cases.STICKY)
def test_sticky_chains_are_repaired(name):
    c = cases.STICKY[name]()
    lnp, z, end, diag, o = held(name, c, **CHUNK)
    print(f"{name}: diag = {diag.tolist()}")
    assert diag[0] >= 1 and diag[1] >= 1
    assert diag.tolist() == ho.restate(c["x"], c["a"], c["w0"], c["mu"], c["nu"], c["u"], **CHUNK)[3].tolist()


@pytest.mark.parametrize("name", sorted(cases.HARD) + ["zero_start_entries", "k8_d33_cond1e4"])
def test_hard_cases_and_a_start_with_zero_entries(name):
    c = cases.RECIPES[name]()
    lnp, z, end, diag, o = held(name, c, **CHUNK)
    if name == "zero_start_entries":
        assert np.count_nonzero(c["w0"] == 0.0) == 2 and o.phi[0, 0] == 0.0 and np.all(np.isfinite(lnp))


# ---- slicing and continuation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", ((130,), (70, 200)))
def test_a_sequence_in_slices_joined_by_phi_a(cuts):
    """Whole against slices each started from ``end @ A`` of the slice before.  Both are within 2 B of their own oracles, and
    the two oracles differ by at most the projective error of the start handed over (the recursion is non-expansive): the
    2 H the slices before have accumulated."""
    c = cases.make(3, 2, 300, 304)
    eng = engine(3, 2)
    whole, _, end_whole, _, _ = run(c, eng=eng, **CHUNK)
    ow = ho.exact_of(eng.last, c["x"])
    check("whole", ow, whole, None, end_whole)
    w, lo, handed = c["w0"], 0, 0.0
    for hi in list(cuts) + [300]:
        part, _, end, _, _ = run(c, c["x"][lo:hi], eng=eng, w0=w, pivot=c["x"][0], **CHUNK)
        op = ho.exact_of(eng.last, c["x"][lo:hi])
        assert np.all(np.abs(part - whole[lo:hi]) <= 2.0 * (op.B + ow.B[lo:hi]) + handed), (lo, hi)
        handed += 2.0 * op.H[-1]                                  # (what this slice's end vector carries on)
        w, lo = end @ c["a"], hi
    assert np.all(np.abs(end - end_whole) <= (handed + 2.0 * ow.H[-1]) * end_whole + 1e-300)


# ---- agreement with existing code ---------------------------------------------------------------------------------------
def test_one_row_is_the_student_t_mixture_with_the_start_as_weights():
    from bayesml_amd import _stmix
    c = cases.make(5, 17, 1, 305)
    lnp, z, end, diag, o = held("T = 1", c)
    mix = _stmix.StudentMixturePass(5, 17, DEV)
    got, _ = mix.run(mix.adopt(c["x"]), c["w0"], c["mu"], c["nu"], c["u"], False)
    om = so.exact(c["u"], c["mu"], c["nu"], c["w0"], c["x"][0], c["x"])
    assert abs(float(got[0]) - lnp[0]) <= 2.0 * (om.B[0] + o.B[0])


def test_a_duplicated_state_yields_the_lower_index():
    c = cases.duplicate_state(cases.make(4, 3, 200, 306), 1, 3)
    for kw in (CHUNK, {}):
        lnp, z, end, diag, _ = run(c, **kw)
        assert end[1] == end[3] and 3 not in z and 1 in z


def numpy_filter(m, x, w0):
    from scipy.special import logsumexp
    from scipy.stats import multivariate_t
    p = m.get_p_params()
    K = m.c_num_classes
    le = np.stack([multivariate_t(loc=p["p_mu_vecs"][k], shape=np.linalg.inv(p["p_lambda_mats"][k]), df=p["p_nus"][k]).logpdf(x)
                   for k in range(K)], axis=1)
    w, lnp, phi = np.asarray(w0, dtype=np.float64), np.empty(len(x)), np.empty((len(x), K))
    for t in range(len(x)):
        lt = np.log(w) + le[t]
        lnp[t] = logsumexp(lt)
        phi[t] = np.exp(lt - lnp[t])
        w = phi[t] @ p["p_a_mat"]
    return lnp, phi


@pytest.mark.parametrize("K, D, T", ((3, 2, 1000), (4, 33, 2000)))
def test_after_a_real_fit_against_a_numpy_filter(K, D, T):
    import warnings
    from bayesml_amd import _hmmpred, hiddenmarkovnormal as hm
    rng = np.random.default_rng(K)
    a = np.full((K, K), 0.2 / (K - 1))
    np.fill_diagonal(a, 0.8)
    gen = hm.GenModel(K, D, a_mat=a, mu_vecs=4.0 * rng.standard_normal((K, D)), seed=1)
    x, _ = gen.gen_sample(T, device=DEV)
    xh = x.cpu().numpy()
    m = hm.LearnModel(K, D, seed=0, device=DEV, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.update_posterior(x, max_itr=20, num_init=1)
    kept = {k: v.copy() for k, v in m.get_hn_params().items()}
    gamma_last = m.gamma_vecs[-1].copy()
    fit_engine = m._engine
    for start, w0 in (("last", None), ("initial", None)):
        lnp, z, state = m.calc_pred_logpdf(xh, start=start, assign=True, return_state=True)
        w0 = gamma_last @ m.p_a_mat if start == "last" else m.hn_eta_vec / m.hn_eta_vec.sum()
        want, phi = numpy_filter(m, xh, w0)
        err = float(np.max(np.abs(lnp - want) / (1.0 + np.abs(want))))
        print(f"K = {K}, D = {D}, T = {T}, start = {start}: max |ln p - NumPy| / (1 + |ln p|) = {err:.2e}; sum ln p = {lnp.sum():.6f}")
        assert isinstance(lnp, np.ndarray) and err <= 1e-9
        top = np.sort(phi, axis=1)
        clear = top[:, -1] - top[:, -2] > 1e-9
        assert np.array_equal(z[clear], phi.argmax(axis=1)[clear]) and np.allclose(state, phi[-1], rtol=1e-8, atol=1e-12)
        tl, tz = m.calc_pred_logpdf(x, start=start, assign=True)                    # the device tensor, read in place
        assert isinstance(tl, torch.Tensor) and tl.device == x.device and tz.dtype == torch.int64
        assert np.array_equal(tl.cpu().numpy(), lnp) and np.array_equal(tz.cpu().numpy(), z)
        budget = 8 * _hmmpred.scratch_len(K, D, T // 3)
        cut = m.calc_pred_logpdf(xh, start=start, chunk_bytes=budget)                # three or more time slices
        assert np.all(np.abs(cut - want) <= 1e-9 * (1.0 + np.abs(want)))
    assert m._engine is fit_engine and all(np.array_equal(v, m.get_hn_params()[k]) for k, v in kept.items())
    assert np.array_equal(m.gamma_vecs[-1], gamma_last)
