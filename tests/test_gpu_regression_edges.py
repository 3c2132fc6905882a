"""The regression data passes (csrc/regvb_kernels.h: gram_kernel with both row sources, pack_factor_kernel, predict_kernel)
on the GPU at every tile count T = 2 .. 16 and at the edges of their branches (regression_exact_cases.py).

A. Exact inputs: the device block equals an int64 reference with ``np.array_equal``.  The statistics run at both ends of
   every T with three and with four batches of 16 rows per split (the prefetch loop returns to its first buffer), the last
   split cut to 1, 15, 16, 17 or 33 rows, f32 / f64 / mixed dtypes, contiguous and strided rows with NaN in the pad columns;
   the lag window at p = 64 .. 255, both paddings; the read-out at both workgroup heights with NaN in the pad columns and in
   the strict upper triangle of the factor.
B. Badly scaled real inputs: every entry within the derived bound of regression_exact_cases.py of a longdouble reference.
C. linearregression and autoregressive at T = 6, 12, 14 against regression_oracle at the lines of test_gpu_regression.py.

Every test of B prints worst error / bound; the measured figures are in DESIGN.md ("Regression data passes: what the tests
hold").
"""
import numpy as np
import pytest
import torch

import regression_exact_cases as cases
import regression_oracle as orc
from conftest import rel_err

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
WINDOW_PS = (64, 95, 96, 127, 128, 159, 191, 223, 254, 255)
PREDICT_NS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4097)      # workgroups of 64 rows (T > 10) and of 128
BOUND_DS = (17, 49, 80, 127, 129, 176, 208, 255)                  # one per T
SCALE = 1.75


def dev():
    return torch.device("cuda", 0)


def engine(D):
    from bayesml_amd._regression import RegressionPass
    return RegressionPass(D, dev())


def on_device(values, dtype, strided):
    """Rows [N, D] on the device; ``strided``: a view of a [N, D + 3] buffer whose three pad columns are NaN."""
    values = np.asarray(values, dtype=dtype)
    if not strided:
        return torch.from_numpy(np.ascontiguousarray(values)).to(dev())
    buf = np.full((values.shape[0], values.shape[1] + 3), np.nan, dtype=dtype)
    buf[:, :values.shape[1]] = values
    t = torch.from_numpy(buf).to(dev())[:, :values.shape[1]]
    assert values.shape[0] == 1 or t.stride(0) == values.shape[1] + 3
    return t


def test_restated_launch_plan_is_the_library_s():
    """regvb_stats_work_len is gram_max_splits(T) slabs: the split rule the cases are built on is the compiled one."""
    from bayesml_amd._regression import load_library
    lib = load_library()
    for D in cases.STATS_DS:
        T = cases.even_tiles(D)
        assert lib.regvb_stats_work_len(D) == cases.gram_max_splits(T) * cases.gram_slab_len(T), D


# ---- A: exact inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,batches,last,N", cases.stats_grid(), ids=lambda v: str(v))
def test_exact_stats_with_three_and_four_batches_per_split(D, batches, last, N):
    """Bit for bit, n included.  (rps, S, last) as launch_gram computes them are asserted first: every split but the last
    holds ``batches`` batches, so ``more`` is true twice or three times and the loop deposits into buffer 0 again."""
    T = cases.even_tiles(D)
    rps = -(-N // cases.gram_max_splits(T))
    rps = -(-rps // 16) * 16
    S = -(-N // rps)
    assert (rps, N - (S - 1) * rps) == (16 * batches, last) and 1 < S <= cases.gram_max_splits(T)
    a, b, e = cases.matrix_case(D, N, 1000 * batches + D)
    ref = cases.stats_reference(a, b, e, cases.E_Y)
    eng = engine(D)
    dtypes = [(F32, F32), (F64, F64)] + ([(F32, F64), (F64, F32)] if D in cases.MIXED_DS else [])
    for xt, yt in dtypes:
        x, yd = cases.scaled(a, e, xt), torch.from_numpy(cases.scaled(b, cases.E_Y, yt)).to(dev())
        for strided in (False, True):
            s = eng.stats(eng.adopt(on_device(x, xt, strided)), yd).cpu().numpy()
            assert not np.isnan(s).any(), ("a pad column leaked", xt, yt, strided)
            assert np.array_equal(s, ref), (xt, yt, strided, int(np.sum(s != ref)))


@pytest.mark.parametrize("D", cases.STATS_DS)
def test_exact_stats_on_short_samples(D):
    """The same on single-batch splits: one split of 1, 15 or 16 rows, and two and three splits with one row in the last:
    bit for bit at both ends of every T, strided f32 and contiguous f64."""
    eng = engine(D)
    a, b, e = cases.matrix_case(D, 33, 1500 + D)
    for N in (1, 15, 16, 17, 33):
        assert cases.split_plan(N, cases.even_tiles(D)) == (16, -(-N // 16), (N - 1) % 16 + 1)
        ref = cases.stats_reference(a[:N], b[:N], e, cases.E_Y)
        for dt, strided in ((F32, True), (F64, False)):
            yd = torch.from_numpy(cases.scaled(b[:N], cases.E_Y, dt)).to(dev())
            s = eng.stats(eng.adopt(on_device(cases.scaled(a[:N], e, dt), dt, strided)), yd).cpu().numpy()
            assert np.array_equal(s, ref), (N, dt, int(np.sum(s != ref)))


@pytest.mark.parametrize("p", WINDOW_PS)
def test_exact_window_stats(p):
    """The lag-window source at T = 6 .. 16: one row, two rows, a cut second batch and splits of three batches, both paddings,
    bit for bit.  Under zero padding the length p + 1 holds the p rows that reach into negative times and one full row; at
    the long series those p rows are also what the two paddings differ by, exactly."""
    from bayesml_amd._regression import PAD_NONE, PAD_ZEROS
    T = cases.even_tiles(p + 1)
    long = 32 * cases.gram_max_splits(T) + 1 + p
    ints = cases.series_case(long, 2000 + p)
    eng = engine(p + 1)
    series = {dt: torch.from_numpy(cases.scaled(ints, cases.E_SERIES, dt)).to(dev()) for dt in (F32, F64)}
    for length in (p + 1, p + 2, p + 17, long):
        got = {}
        for code, padding in ((PAD_NONE, None), (PAD_ZEROS, "zeros")):
            n_rows = length - (0 if padding else p)
            if length == long:
                assert cases.split_plan(n_rows, T)[0] == 48
            ref = cases.window_reference(ints[:length], p, padding)
            for dt in (F32, F64):
                s = eng.stats_window(series[dt][:length], code).cpu().numpy()
                assert s[-1] == n_rows and np.array_equal(s, ref), (length, padding, dt, int(np.sum(s != ref)))
            got[padding] = s
        if p > 0:
            head = cases.window_reference(ints[:length], p, "zeros", rows=slice(0, p))
            assert np.array_equal(got["zeros"] - got[None], head), length


@pytest.mark.parametrize("D", cases.STATS_DS)
def test_exact_predict(D):
    """p_ms bit for bit; p_lambdas equal to NumPy's ``scale / (1 + q)`` on the exact q, a single correctly rounded division
    on both sides (measured: no entry differs at any D, N or dtype, so equality is asserted, not one ulp).  The rows are
    strided with NaN pads and the factor carries NaN above its diagonal; a second run on contiguous rows and a clean factor
    gives the same bits."""
    Li, xi, mui = cases.predict_case(D, max(PREDICT_NS), 3000 + D)
    m, q = cases.predict_reference(Li, xi, mui)
    want = SCALE / (1.0 + q)
    linv, mu = Li / 8.0, mui.astype(F64)
    dirty = linv.copy()
    dirty[np.triu_indices(D, 1)] = np.nan
    eng = engine(D)
    for N in PREDICT_NS:
        for dt in (F32, F64):
            pm, pl = eng.predict(eng.adopt(on_device(xi[:N], dt, True)), mu, dirty, SCALE)
            pm2, pl2 = eng.predict(eng.adopt(on_device(xi[:N], dt, False)), mu, linv, SCALE)
            assert torch.equal(pm, pm2) and torch.equal(pl, pl2), (N, dt)
            pm, pl = pm.cpu().numpy(), pl.cpu().numpy()
            assert np.array_equal(pm, m[:N]), (N, dt)
            off = np.abs(pl - want[:N]) / np.spacing(want[:N])
            if off.max() > 0:
                print(f"predict exact D = {D} N = {N} {dt.__name__}: {int(np.sum(off > 0))} of p_lambdas off, worst {off.max()} ulp")
            assert np.array_equal(pl, want[:N]), (N, dt, off.max())


# ---- B: derived bounds on badly scaled data ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (17, 4097))
@pytest.mark.parametrize("D", BOUND_DS)
def test_scaled_stats_within_the_derived_bound(D, N):
    """Every entry of G, c and s within (rps + S + 4) u sum |w_ni w_nj| of the longdouble sums of the values as given."""
    T = cases.even_tiles(D)
    x64, y64 = cases.scaled_rows(D, N, 4000 + D)
    eng = engine(D)
    for dt in (F64, F32):
        x, y = x64.astype(dt), y64.astype(dt)
        ref, mag = cases.hp_stats(x, y)
        s = eng.stats(eng.adopt(x), eng.adopt(y)).cpu().numpy()
        ratio = cases.err(s[:-1], ref) / cases.stats_bound(mag, N, T)
        G = ratio[:D * D].reshape(D, D)
        print(f"stats bound D = {D} N = {N} {dt.__name__}: worst error / bound  G {G.max():.3f}  c {ratio[D * D:-1].max():.3f}  "
              f"s {ratio[-1]:.3f}  (depth {cases.split_plan(N, T)[0] + cases.split_plan(N, T)[1] + 4})")
        assert s[-1] == N and ratio.max() <= 1.0, (dt, np.unravel_index(np.argmax(G), G.shape), ratio.max())


@pytest.mark.parametrize("N", (17, 4097))
@pytest.mark.parametrize("D", BOUND_DS)
def test_scaled_predict_within_the_derived_bound(D, N):
    """The read-out against the SAME factor evaluated in longdouble (not against solve()), the factor that of a Lambda with
    condition number about 1e8: p_ms within gamma_(D+2) sum |x_f mu_f|, p_lambdas within |dq| / (1 + q) + 2 u relatively."""
    from bayesml_amd._normalgamma import inverse_factor
    lam, mu, scales = cases.conditioned_factor(D, 5000 + D)
    assert 1e7 < np.linalg.cond(lam) < 1e9
    linv = inverse_factor(lam)
    x64 = cases.conditioned_rows(D, N, 6000 + D, scales)
    eng = engine(D)
    for dt in (F64, F32):
        x = x64.astype(dt)
        m, lam_ref, bound_m, bound_l = cases.hp_predict(x, mu, linv, SCALE)
        pm, pl = (t.cpu().numpy() for t in eng.predict(eng.adopt(x), mu, linv, SCALE))
        rm = cases.err(pm, m) / bound_m
        rl = cases.err(pl, lam_ref) / (bound_l * np.asarray(lam_ref, dtype=F64))
        print(f"predict bound D = {D} N = {N} {dt.__name__}: worst error / bound  p_ms {rm.max():.3f}  p_lambdas {rl.max():.3f}  "
              f"(relative bound on p_lambdas up to {bound_l.max():.2e})")
        assert rm.max() <= 1.0 and rl.max() <= 1.0, (dt, rm.max(), rl.max())


# ---- C: the models at the tile counts no other test reaches -----------------------------------------------------------------
@pytest.mark.parametrize("D", (80, 176, 208))
def test_linreg_model_at_six_twelve_and_fourteen_tiles(D):
    from bayesml_amd import linearregression as lr
    x, y, _theta = orc.synth_linreg(D, 400, 7000 + D, 2.0, F64)
    m = lr.LearnModel(D, device=dev()).update_posterior(x, y)
    mu, lam, alpha, beta = orc.update(np.zeros(D), np.eye(D), 1.0, 1.0, x, y)
    assert rel_err(m.hn_lambda_mat, lam) < 1e-12 and rel_err(m.hn_mu_vec, mu) < 1e-10
    assert m.hn_alpha == alpha and rel_err(m.hn_beta, beta) < 1e-10
    pm, pl, pn = orc.pred_params(mu, lam, alpha, beta, x[:150])
    got = m.predict(x[:150])
    assert rel_err(got, pm) < 1e-10 and rel_err(m.p_ms, pm) < 1e-10 and rel_err(m.p_lambdas, pl) < 1e-10
    assert np.array_equal(m.p_nus, pn)


@pytest.mark.parametrize("p", (79, 175, 207))
def test_ar_model_at_six_twelve_and_fourteen_tiles(p):
    from bayesml_amd import autoregressive as ar
    rng = np.random.default_rng(8000 + p)
    e = rng.standard_normal(p + 501)
    x = 0.3 + e[1:] + 0.6 * e[:-1]
    for padding in (None, "zeros"):
        m = ar.LearnModel(p, device=dev()).update_posterior(x, padding=padding)
        w, y = orc.lag_matrix(x, p, padding)
        mu, lam, alpha, beta = orc.update(np.zeros(p + 1), np.eye(p + 1), 1.0, 1.0, w, y)
        assert rel_err(m.hn_lambda_mat, lam) < 1e-12 and rel_err(m.hn_mu_vec, mu) < 1e-10, padding
        assert m.hn_alpha == alpha and rel_err(m.hn_beta, beta) < 1e-10, padding
