"""The Student-t mixture log-density on the device (include/stmix.h) against the exact oracle of tests/stmix_oracle.py: every
ln p_i within 2 B_i of the exact value (B_i: the derived bound there; 2 is its only margin), the arg-max equal to the
oracle's wherever the two largest t_ik differ by more than 2 (B_ik + B_ik'), rows independent of each other bit for bit,
nothing written past the end.  Shapes are the smallest at which a path can go wrong: the exact oracle costs K N D^2 integer
products.  Every test prints its worst |error| / B_i (profiles/stmix.md has them): measured 0.001 to 0.14 over all cases,
the largest at nu_across_lgamma_threshold; the model tests 0.02 of their tolerance and below.

Tiles (csrc/stmix_kernels.h): a wave holds 16 NB rows with NB = max(1, min(4, 8 / T) / 2), a workgroup 8 waves; component
images go through LDS in blocks of estep_kb(T) = 16, 9, 4, 3, 2, 1, 1, 1 for T = 1 .. 8 feature tiles.
"""
import numpy as np
import pytest
import torch

import stmix_cases as cases
import stmix_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KB = {1: 16, 2: 9, 3: 4, 4: 3, 5: 2, 6: 1, 7: 1, 8: 1}           # estep_kb(T)


def wave_rows(T):
    return 16 * max(1, min(4, 8 // T) // 2)


def engine(K, D):
    from bayesml_amd import _stmix
    return _stmix.StudentMixturePass(K, D, DEV)


def run(c, x=None, want_z=True, eng=None):
    """(ln p, z) as NumPy arrays for the rows ``x`` (default: the case's, float64) under the case's parameters."""
    K, D = c["mu"].shape
    eng = eng or engine(K, D)
    xd = eng.adopt(c["x"] if x is None else x)
    lnp, z = eng.run(xd, c["pi"], c["mu"], c["nu"], c["u"], want_z)
    torch.cuda.synchronize()
    return lnp.cpu().numpy(), (z.cpu().numpy() if want_z else None)


def held(label, c, lnp, z, x=None):
    """The engine's results against the oracle built from what the engine was handed."""
    x = c["x"] if x is None else x
    o = so.exact(c["u"], c["mu"], c["nu"], c["pi"], np.asarray(x[0], dtype=np.float64), x)
    worst, at = o.ratio(lnp)
    print(f"{label}: worst |error| / B_i = {worst:.3f} at row {at} of {len(lnp)}")
    assert worst <= 2.0, (label, worst, at)
    decided = o.z_decided()
    assert np.array_equal(z[decided], o.z[decided]), label
    assert z.min() >= 0 and z.max() < len(c["pi"])
    return o


# ---- shape edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 2, 15, 16, 17, 32, 33, 48, 64, 100, 128, 129, 200))
def test_every_feature_tile_count_and_the_plain_path(D):
    """Every T, the zero-padded last block and the scalar-load path (D no multiple of 16), the plain kernel above 128."""
    c = cases.make(3, D, 40 if D <= 128 else 20, 100 + D)
    held(f"D = {D}", c, *run(c))


@pytest.mark.parametrize("T", (1, 2, 4, 8))
def test_component_blocks_and_row_tiles(T):
    """K around the LDS block (partial and several blocks; at T = 8 a block is one component) taken pairwise with N around
    the wave tile and the workgroup tile; each N takes the next K in turn that the oracle can afford."""
    D = 16 * T
    wave = wave_rows(T)
    ks = sorted({1, 2, max(KB[T] - 1, 1), KB[T], KB[T] + 1, 33}, reverse=True)
    ns = sorted({1, 15, 16, 17, wave - 1, wave, wave + 1, 8 * wave - 1, 8 * wave, 8 * wave + 1, 1000})
    big = cases.make(33, D, 1000, 200 + T)
    for i, n in enumerate(ns):
        turn = ks[i % len(ks):] + ks[:i % len(ks)]
        K = next((k for k in turn if k * n * D * D <= 1.2e7), 1)          # (the oracle's cost: a few seconds per T in all)
        c = {key: big[key][:K] for key in ("mu", "nu", "u")}
        c["pi"] = big["pi"][:K] / big["pi"][:K].sum()
        c["x"] = big["x"][:n]
        held(f"T = {T}, K = {K}, N = {n}", c, *run(c))


# ---- storage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (16, 20))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_storage_does_not_change_a_bit(D, dtype):
    """ldx = D (vector loads at D = 16), ldx = D + 3 and a view one element in (scalar loads), ldx = D + 4 (vector loads,
    strided), a NumPy sample: the same rows give the same bits, and they meet the bound."""
    c = cases.make(3, D, 70, 300 + D, f32=True)
    K, n = 3, 70
    eng = engine(K, D)
    x = torch.from_numpy(c["x"].astype(dtype)).to(DEV)
    base_l, base_z = run(c, x, eng=eng)
    held(f"D = {D}, {np.dtype(dtype).name}, ldx = D", c, base_l, base_z)
    wide3 = torch.zeros(n, D + 3, dtype=x.dtype, device=DEV)
    wide3[:, :D] = x
    wide4 = torch.zeros(n, D + 4, dtype=x.dtype, device=DEV)
    wide4[:, :D] = x
    flat = torch.zeros(n * D + 1, dtype=x.dtype, device=DEV)
    flat[1:] = x.reshape(-1)
    shifted = flat[1:].view(n, D)
    assert shifted.data_ptr() % 16 != 0 and wide3[:, :D].stride(0) == D + 3
    for label, xs in (("ldx = D + 3", wide3[:, :D]), ("ldx = D + 4", wide4[:, :D]), ("one element in", shifted),
                      ("NumPy", c["x"].astype(dtype))):
        l, z = run(c, xs, eng=eng)
        assert np.array_equal(l, base_l) and np.array_equal(z, base_z), label


# ---- rows are independent --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, K", ((16, 17), (128, 3), (130, 2)))
def test_a_row_does_not_depend_on_the_other_rows(D, K):
    T = (D + 15) // 16
    wave = wave_rows(min(T, 8))
    n_all = 1000 if D <= 128 else 150
    c = cases.make(K, D, n_all, 400 + D)
    eng = engine(K, D)
    whole_l, whole_z = run(c, eng=eng)
    again_l, again_z = run(c, eng=eng)
    assert np.array_equal(whole_l, again_l) and np.array_equal(whole_z, again_z)          # two runs
    assert np.all(np.isfinite(whole_l))
    for n in sorted({1, 15, 16, 17, wave - 1, wave, wave + 1, 8 * wave - 1, 8 * wave, 8 * wave + 1, 64, 65}):
        if n >= n_all:
            continue
        # (the pivot is row 0 of either sample)
        l, z = run(c, c["x"][:n], eng=eng)
        assert np.array_equal(l, whole_l[:n]) and np.array_equal(z, whole_z[:n]), n


# ---- nothing past the end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (16, 40, 129))
def test_nothing_is_written_past_the_end(D):
    """stmix_logpdf called directly with outputs longer than n_rows, filled with sentinels; with and without z."""
    from bayesml_amd import _stmix
    lib = _stmix.load_library()
    K = 3
    c = cases.make(K, D, 300, 500 + D)
    eng = engine(K, D)
    ref_l, ref_z = run(c, eng=eng)                               # (also leaves the packed image and its pivot in eng)
    last = eng.last
    x = torch.from_numpy(c["x"]).to(DEV)
    for n in (1, 17, 127, 129, 257):
        for with_z in (True, False):
            lnp = torch.from_numpy(np.full(n + 300, 0x7FF8DEADBEEF0001, dtype=np.uint64).view(np.float64)).to(DEV)
            z = torch.full((n + 300,), -7, dtype=torch.int64, device=DEV)
            rc = lib.stmix_logpdf(K, D, 1, x.data_ptr(), D, n, last["pivot"].data_ptr(), eng.img.data_ptr(), last["c"].data_ptr(),
                                  last["nu"].data_ptr(), lnp.data_ptr(), z.data_ptr() if with_z else None, None)
            assert rc == 0, lib.stmix_last_error()
            torch.cuda.synchronize()
            got = lnp.cpu().numpy()
            assert np.array_equal(got[:n], ref_l[:n])
            assert np.all(got[n:].view(np.uint64) == np.uint64(0x7FF8DEADBEEF0001))
            zs = z.cpu().numpy()
            assert np.all(zs[n:] == -7) and (np.array_equal(zs[:n], ref_z[:n]) if with_z else np.all(zs[:n] == -7))


# ---- hard numerics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.RECIPES)
def test_recipes(name):
    """Far means about a row-0 pivot, rows exactly at a mean, outliers with q / nu >= 1e12, nu across the lnGamma threshold,
    weights down to 1e-300, every t below -1e5 (ln p finite), condition 1e6 (tests/test_stmix.py asserts the branches)."""
    c = cases.RECIPES[name]()
    lnp, z = run(c)
    assert np.all(np.isfinite(lnp))
    held(name, c, lnp, z)


@pytest.mark.parametrize("D", (64, 128))
def test_degrees_of_freedom_one_and_1e8(D):
    """p_nu = 1 (hn_nus = D) beside p_nu = 1e8."""
    c = cases.make(2, D, 16, 600 + D, nu=np.array([1.0, 1e8]))
    held(f"nu = 1 and 1e8, D = {D}", c, *run(c))


# ---- assign ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (16, 129))
def test_a_duplicated_component_yields_the_lower_index(D):
    c = cases.duplicate_component(cases.make(4, D, 60, 700 + D), 1, 3)
    c["x"][4:30] = c["mu"][1] + 0.5 * np.random.default_rng(D).standard_normal((26, D))      # rows that belong to it
    lnp, z = run(c)
    o = held(f"duplicate, D = {D}", c, lnp, z)
    assert np.array_equal(o.t[:, 1], o.t[:, 3])
    assert not np.any(z == 3) and np.sum(z == 1) >= 20


# ---- the models --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, D, N", ((3, 2, 1000), (4, 33, 2000)))
def test_gaussianmixture_after_a_fit(K, D, N):
    import warnings
    from bayesml_amd import gaussianmixture as gm
    from oracle import gmm_vb_oracle as orc
    x = orc.synth_gmm(K, D, N + 500, np.float64)
    m = gm.LearnModel(K, D, seed=0, device=DEV, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.update_posterior(x[:N], max_itr=20, num_init=1)
    keep = {k: v.copy() for k, v in m.get_hn_params().items()}
    r = m.r_vecs.copy()
    eng = m._engine
    fresh = x[N:]
    lnp, z = m.calc_pred_logpdf(fresh, assign=True)
    assert isinstance(lnp, np.ndarray) and lnp.shape == (500,) and z.dtype == np.int64
    p = m.get_p_params()
    want, cond = so.exact_from_precision(p["p_lambda_mats"], p["p_mu_vecs"], p["p_nus"], m.hn_alpha_vec / m.hn_alpha_vec.sum(), fresh)
    tol = so.model_tolerance(D, cond, want)
    print(f"K = {K}, D = {D}: worst |error| / tolerance = {np.max(np.abs(lnp - want) / tol):.3f}, cond up to {cond.max():.1e}")
    assert np.all(np.abs(lnp - want) <= tol)
    for k, v in m.get_hn_params().items():
        assert np.array_equal(v, keep[k]), k
    assert np.array_equal(m.r_vecs, r) and m._engine is eng
    td = m.calc_pred_logpdf(torch.from_numpy(fresh).to(DEV))
    assert isinstance(td, torch.Tensor) and td.device == torch.device(DEV) and np.array_equal(td.cpu().numpy(), lnp)


@pytest.mark.parametrize("D", (1, 16, 33))
def test_multivariate_normal_after_an_update(D):
    from bayesml_amd import multivariate_normal as mvn
    rng = np.random.default_rng(D)
    a = rng.standard_normal((D, D)) / np.sqrt(D)
    x = 5.0 + rng.standard_normal((1500, D)) @ (a + np.eye(D))
    m = mvn.LearnModel(D, device=DEV).update_posterior(x[:1000])
    keep = {k: np.copy(v) for k, v in m.get_hn_params().items()}
    lnp = m.calc_pred_logpdf(x[1000:])
    want, cond = so.exact_from_precision(m.p_v_mat[None], m.p_m_vec[None], [m.p_nu], [1.0], x[1000:])
    tol = so.model_tolerance(D, cond, want)
    print(f"D = {D}: worst |error| / tolerance = {np.max(np.abs(lnp - want) / tol):.3f}, cond {cond.max():.1e}")
    assert lnp.shape == (500,) and np.all(np.abs(lnp - want) <= tol)
    for k, v in m.get_hn_params().items():
        assert np.array_equal(v, keep[k]), k
