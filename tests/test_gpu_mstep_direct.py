"""The M-step's direct-weight modes - an HMM pass (r = gamma, h = sum gamma ln rho) and loaded responsibilities
(h = sum r ln r) - through the C ABI at every emission degree: the per-component raw sums ns, a, B, h of every M-step kernel
family against a long-double evaluation of the same sums (tests/mstep_direct_reference.py).

The reference takes the DEVICE's weights (responsibilities(), ln_rho(), pivot), so that a failure here is the M-step's and not
a rounding difference of the forward-backward pass; gamma itself is held to the oracle's forward-backward once per case
(absolute 1e-10, as tests/test_gpu_hmm.py).  The bound is derived, not measured: both sides add the same binary64 products
in another order and the device rounds w xc once before the MFMA, so per entry and per component
    |device - reference| <= (N + 8) 2^-53 sum_t |term_t|.
A dropped or misplaced row costs about one term in N: ten orders of magnitude above the bound.

Every HMM case also asserts the kernel named by launch_info (a dispatch change that reroutes a shape fails here), h = 0 and
bit-identical ns, a, B under hmmvb_skip_h, and bit-identical statistics on a second run.

Two things the kernels decide that the cases follow:
* one feature tile has no vector-load form (mstep_inst.hip: T in {2, 4, 8}), so unprepared rows of D = 16 report `masked`;
* hmm_mstep_small leaves terms with gamma < 2^-80 out of a and B unless GMMVB_HMM_MSTEP_DENSE is set: the bound on a and B is
  asserted for the dense walk, ns and h (complete sums in both) for both.
mstep_small_f64 with direct_r == 2 is not reachable from the C ABI (prepared one-tile HMM passes all take hmm_mstep_small).

Worst |device - reference| / bound per kernel family over the cases below, as they print it on an MI355X (the kernels are
run-to-run deterministic, so these repeat):
                                                      ns       a        B        h
    HMM     mstep_mfma_f64<T=2..8,centred-f64>        0.020    0.035    0.107    0.079
            mstep_mfma_f64<T=1..8,x=..,masked>        0.022    0.033    0.096    0.019
            mstep_mfma_f64<T=2|4|8,x=..,vec>          0.021    0.029    0.096    0.018
            mstep_wide_f64<T=10..16>                  0.0043   0.013    0.017    0.0077
            mstep_generic_f64                         0.018    0.025    0.058    0.012
            hmm_mstep_small, every step               0.0028   0.0099   0.027    0.0047
            hmm_mstep_small, steps above 2^-80        0.0028   3.4e13   3.4e13   0.0047   (a, B: by design, not asserted)
    loaded  mstep_mfma_f64<T=2|8,centred-f64>         0.0040   0.0024   0.014    0.0038
            mstep_mfma_f64<T=3,x=f64,masked>          0.0094   0.014    0.070    0.024
            mstep_mfma_f64<T=4,x=f32,vec>             0.0041   0.0028   0.017    0.0055
            mstep_wide_f64<T=10>                      0.0025   0.00081  0.0064   0.0020
            mstep_generic_f64                         0.0089   0.0072   0.057    0.021
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import mstep_direct_reference as ref
from conftest import rel_err
from oracle import hmm_vb_oracle as orc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


# ---- inputs: the recipe of tests/test_gpu_hmm.py::test_ragged_shapes_against_oracle ------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_inputs(K, D, N, dtype):
    """(x, random posterior, the oracle's gamma) - computed once per shape, shared by the cases, never written to."""
    rng = np.random.default_rng(100 * K + D)
    x, _ = orc.synth_hmm(max(2, K // 2), D, N, dtype, seed=K + N, stay=0.8)
    p = orc.HmmPrior.default(K, D)
    q = orc.HmmPosterior.from_prior(p)
    q.m = 3.0 * rng.standard_normal((K, D))
    a = rng.standard_normal((K, D, D))
    q.w_inv = a @ np.swapaxes(a, 1, 2) + D * np.eye(D)
    q.w = np.linalg.inv(q.w_inv)
    q.nu = q.nu + rng.uniform(0, 3, K)
    q.kappa = q.kappa + rng.uniform(0, 3, K)
    q.eta = q.eta + rng.uniform(0, 5, K)
    q.zeta = q.zeta + rng.uniform(0, 5, (K, K)) + 4 * np.eye(K)
    q.refresh()
    ln_rho = orc.emission_ln_rho(x.astype(np.float64), q)
    mx = ln_rho.max(axis=1, keepdims=True)
    alpha, beta, _cs = orc.forward_backward(np.exp(ln_rho - mx), q.pi_tilde, q.a_tilde)   # shifted: no underflow
    gamma = alpha * beta
    for arr in (x, gamma):
        arr.setflags(write=False)
    return x, q, gamma


def on_device(x, dev, ldx=None):
    """x on the GPU: contiguous, or (ldx) the leading D columns of a wider buffer whose other columns are NaN."""
    xd = torch.from_numpy(np.array(x)).to(dev)          # (a copy: the shared array is read-only)
    if ldx is None:
        return xd
    buf = torch.full((x.shape[0], ldx), float("nan"), dtype=xd.dtype, device=dev)
    buf[:, :x.shape[1]] = xd
    return buf[:, :x.shape[1]]


def tiles(D):
    return (D + 15) // 16


def check_sums(tag, eng, stats, x, w, h_ref, n_rows):
    """ns, a, B, h of `stats` under the bound, against the reference for weights w; returns the worst ratios."""
    ns, h, a, B = (v.cpu().numpy() for v in eng.split_stats(stats))
    sums = ref.weighted_sums(x, eng.pivot.cpu().numpy(), w)
    sums["h"] = h_ref
    ratios = {k: ref.worst_ratio(dict(ns=ns, h=h, a=a, B=B)[k], *sums[k], n_rows) for k in ("ns", "a", "B", "h")}
    print("mstep-direct", tag, " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    return ratios


def hmm_pass(K, D, N, dtype, want, prepare=True, ldx=None, fused_request=False, bound_on=("ns", "a", "B", "h")):
    """One HMM data pass through the C ABI the way tests/test_gpu_hmm.py::device_pass drives it, and every check of the case."""
    from bayesml_amd import _kside
    from bayesml_amd._engine import DataPass
    dev = torch.device("cuda", 0)
    x, q, gamma_ref = ragged_inputs(K, D, N, dtype)
    t = lambda v: torch.as_tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    f = _kside.features(_kside.PostT(torch.ones(K, dtype=torch.float64, device=dev), t(q.m), t(q.kappa), t(q.nu), t(q.w_inv)))
    c = (f.e_ln_lambda_det - D * _kside.LN_2PI - D / f.kappa) / 2.0
    xd = on_device(x, dev, ldx)
    eng = DataPass(K, D, xd.dtype, N, dev)
    try:
        eng.set_pivot(xd[:4096].to(torch.float64).mean(dim=0))
        if prepare:
            eng.prepare_rows(xd)
        if fused_request:
            eng.enable_hmm()
            assert eng.emission_target(True) is False        # (only in effect at one feature tile)
        eng.set_params(c, f.m, f.u)
        eng.estep(xd)
        ln_rho = eng.ln_rho().cpu().numpy()
        eng.enable_hmm()
        eng.forward_backward(t(q.pi_tilde), t(q.a_tilde))
        eng.hmm_skip_h(False)
        with_h = eng.mstep(xd).clone()
        info = eng.launch_info
        assert want in info, info
        gamma = eng.responsibilities().cpu().numpy()
        assert np.max(np.abs(gamma - gamma_ref)) < 1e-10
        if fused_request:
            assert np.array_equal(eng.ln_rho().cpu().numpy(), ln_rho)      # the ln rho array is still served after the pass
        tag = f"hmm K={K} D={D} N={N} {np.dtype(dtype).name} {want}"
        ratios = check_sums(tag, eng, with_h, x, gamma, ref.h_hmm(gamma, ln_rho), N)
        for k in bound_on:
            assert ratios[k] <= 1.0, (k, ratios)
        eng.hmm_skip_h(True)
        no_h = eng.mstep(xd).clone()
        eng.hmm_skip_h(False)
        assert torch.equal(no_h[K:2 * K], torch.zeros(K, dtype=torch.float64, device=dev))
        assert torch.equal(no_h[:K], with_h[:K]) and torch.equal(no_h[2 * K:], with_h[2 * K:])
        again = eng.mstep(xd).clone()
        assert torch.equal(again, with_h)                    # run-to-run identical
    finally:
        eng.close()
    return ratios


# ---- HMM mode (direct_r == 2) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,N,dtype", [(5, 17, 257, F32), (7, 33, 1000, F64), (4, 49, 65, F32), (6, 65, 513, F64),
                                         (3, 81, 63, F32), (6, 100, 1000, F64), (9, 128, 513, F32), (5, 17, 1, F64)])
def test_hmm_prepared_dense(K, D, N, dtype):
    hmm_pass(K, D, N, dtype, f"mstep_mfma_f64<T={tiles(D)},centred-f64>")


@pytest.mark.parametrize("K,D,T,N,dtype,prepare", [(4, 129, 10, 600, F32, True), (3, 161, 12, 257, F64, True),
                                                   (3, 200, 14, 700, F32, True), (2, 256, 16, 513, F64, True),
                                                   # no prepare_rows: the M-step makes the centred copy itself
                                                   (3, 144, 10, 257, F32, False)])
def test_hmm_wide(K, D, T, N, dtype, prepare):
    hmm_pass(K, D, N, dtype, f"mstep_wide_f64<T={T},centred-f64", prepare=prepare)


@pytest.mark.parametrize("K,D,N,dtype", [(2, 257, 300, F32),          # the first feature of the second panel of 256
                                         (2, 330, 300, F64)])
def test_hmm_generic(K, D, N, dtype):
    hmm_pass(K, D, N, dtype, f"mstep_generic_f64<D={D}>")


def unprepared_cases():
    out = []
    for i, D in enumerate([1, 15, 40, 127, 16, 32, 64, 128]):
        K, N = (3, 65) if i % 2 else (5, 257)
        vec = D % 16 == 0 and tiles(D) > 1           # (one feature tile has no vector-load form)
        for dtype in (F32, F64):
            out.append((K, D, N, dtype, None, "vec" if vec else "masked"))
            if D > 16:
                out.append((K, D, N, dtype, D + 3, "masked"))
                if D % 16 == 0:
                    out.append((K, D, N, dtype, D + 16, "vec"))
    return out


@pytest.mark.parametrize("K,D,N,dtype,ldx,form", unprepared_cases())
def test_hmm_unprepared_dense(K, D, N, dtype, ldx, form):
    """Rows straight from the caller's matrix (no gmmvb_prepare_rows): contiguous, and as a view of a wider buffer whose
    row stride keeps (D + 16) or breaks (D + 3) the alignment of the vector loads."""
    hmm_pass(K, D, N, dtype, f"mstep_mfma_f64<T={tiles(D)},x={'f32' if dtype is F32 else 'f64'},{form}>", prepare=False, ldx=ldx)


@pytest.mark.parametrize("K,D,N,dtype,prepare", [(33, 17, 513, F64, True), (33, 17, 513, F32, False),
                                                 (70, 17, 2305, F32, True),       # hmm_wide.h: chunked recursions, ragged last tile
                                                 (130, 20, 400, F64, True)])      # hmm_generic.h
def test_hmm_state_layouts(K, D, N, dtype, prepare):
    """Padded state counts (Kp != K) and the other recursion families: what changes the component-major copy of gamma."""
    want = "centred-f64>" if prepare else f"x={'f32' if dtype is F32 else 'f64'},masked>"
    hmm_pass(K, D, N, dtype, f"mstep_mfma_f64<T={tiles(D)}," + want, prepare=prepare)


def test_hmm_fused_emission_request_past_one_tile():
    """hmmvb_emission_target(1) is refused at D = 17: the pass keeps its ln rho array and h = sum gamma ln rho."""
    hmm_pass(5, 17, 257, F32, "mstep_mfma_f64<T=2,centred-f64>", fused_request=True)


@pytest.mark.parametrize("dense", [True, False], ids=["every step", "steps above 2^-80"])
def test_hmm_prepared_one_tile(dense, monkeypatch):
    """hmm_mstep_small, the only kernel of a prepared pass at D <= 16.  Its default walk leaves gamma < 2^-80 out of a and B
    (not out of ns and h), which the bound does not allow for a component of tiny weight: a and B are held under
    GMMVB_HMM_MSTEP_DENSE."""
    if dense:
        monkeypatch.setenv("GMMVB_HMM_MSTEP_DENSE", "1")
        hmm_pass(5, 16, 257, F32, "hmm_mstep_small<T=1,8 components per wave,gamma time-major>")
    else:
        monkeypatch.delenv("GMMVB_HMM_MSTEP_DENSE", raising=False)
        hmm_pass(5, 16, 257, F32, "hmm_mstep_small<T=1,8 components per wave,gamma time-major,steps above 2^-80>",
                 bound_on=("ns", "h"))


# ---- loaded responsibilities (direct_r == 1) -----------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,N,dtype,prepare,want", [
    (5, 17, 257, F32, True, "mstep_mfma_f64<T=2,centred-f64>"),
    (9, 128, 513, F64, True, "mstep_mfma_f64<T=8,centred-f64>"),
    (5, 64, 257, F32, False, "mstep_mfma_f64<T=4,x=f32,vec>"),
    (3, 40, 65, F64, False, "mstep_mfma_f64<T=3,x=f64,masked>"),
    (4, 129, 600, F32, True, "mstep_wide_f64<T=10,centred-f64"),
    (3, 257, 300, F64, False, "mstep_generic_f64<D=257>")])
def test_loaded_responsibilities(K, D, N, dtype, prepare, want):
    from bayesml_amd._engine import DataPass
    dev = torch.device("cuda", 0)
    x = ragged_inputs(K, D, N, dtype)[0]
    rng = np.random.default_rng(1000 * K + D)
    r = rng.dirichlet(0.3 * np.ones(K), N)
    r[rng.random((N, K)) < 0.2] = 0.0                  # exact zeros, rows not renormalised: log(0) must stay out of h
    r[:, K // 2] = 0.0                                 # (every case has K >= 3) an empty component
    xd = on_device(x, dev)
    rd = torch.from_numpy(r).to(dev)
    eng = DataPass(K, D, xd.dtype, N, dev)
    try:
        eng.set_pivot(xd[:4096].to(torch.float64).mean(dim=0))
        if prepare:
            eng.prepare_rows(xd)
        eng.load_responsibilities(rd)
        stats = eng.mstep(xd).clone()
        assert want in eng.launch_info, eng.launch_info
        assert torch.equal(eng.responsibilities(), rd)       # the loaded bits
        ratios = check_sums(f"loaded K={K} D={D} N={N} {np.dtype(dtype).name} {want}", eng, stats, x, r, ref.h_loaded(r), N)
        assert all(v <= 1.0 for v in ratios.values()), ratios
        for part in eng.split_stats(stats):
            assert float(part[K // 2].abs().max()) == 0.0    # ns_k = a_k = B_k = h_k = 0 exactly
        assert torch.equal(eng.mstep(xd), stats)
    finally:
        eng.close()


# ---- the public class at widths only the random slice reaches ----------------------------------------------------------------
@pytest.mark.parametrize("K,D,T,dtype,want", [(4, 144, 1500, F32, "mstep_wide_f64<T=10"), (2, 260, 600, F64, "generic")])
def test_wide_sequences_through_the_driver(K, D, T, dtype, want):
    """hiddenmarkovnormal.LearnModel.update_posterior against the oracle's trajectory, in the pattern of
    tests/test_gpu_generic.py::test_wide_rows_through_the_driver.  init_type is random_responsibility: with the default,
    sqrt(T) < D subsampled rows give W^-1 of rank sqrt(T) + 1e-5 I, ln rho of order -1e6, and the reference formulation's
    unshifted exp(ln rho) (which the oracle follows on purpose) is 0 / 0 at every step - there is no oracle trajectory."""
    from bayesml_amd import hiddenmarkovnormal as hmm
    x = orc.synth_hmm(K, D, T, np.dtype(dtype))[0]
    kw = dict(max_itr=4, num_init=1, tolerance=0.0, init_type="random_responsibility")
    m = hmm.LearnModel(K, D, seed=0, device="cuda:0", verbose=False)
    p = orc.HmmPrior.default(K, D)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.update_posterior(x, **kw)
        want_q = orc.update_posterior(x.astype(np.float64), p, orc.HmmPosterior.from_prior(p), np.random.default_rng(0), **kw)
    assert want in m._engine.launch_info, m._engine.launch_info
    hn = m.get_hn_params()
    q = want_q.posterior
    for key, val in (("hn_eta_vec", q.eta), ("hn_zeta_vecs", q.zeta), ("hn_m_vecs", q.m), ("hn_kappas", q.kappa),
                     ("hn_nus", q.nu), ("hn_w_mats", q.w)):
        assert rel_err(hn[key], val) < 1e-7, key
    # ... and to rounding for the posterior the model itself holds (the final pass of ref:1133)
    own = orc.HmmPosterior(hn["hn_eta_vec"].copy(), hn["hn_zeta_vecs"].copy(), hn["hn_m_vecs"].copy(), hn["hn_kappas"].copy(),
                           hn["hn_nus"].copy(), hn["hn_w_mats"].copy(), m.hn_w_mats_inv.copy()).refresh()
    st = orc.data_pass(x.astype(np.float64), own)
    assert np.max(np.abs(m.gamma_vecs - st.gamma)) < 1e-9
    assert rel_err(m.ns, st.ns) < 1e-10 and rel_err(m.s_mats, st.s) < 1e-9
