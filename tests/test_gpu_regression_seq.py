"""The sequential regression kernels (csrc/regseq_kernels.h) on the GPU, through ``pred_and_update_sequence`` of both
models and through ``regseq_pass`` itself.

Tolerance (regression_seq_oracle.check): an output is compared with the long-double loop and must lie within 8 x the
reference loop's own error on the same rows, never below 64 eps; relative per row for p_lambda and nats (a code length's magnitude floored at 1),
relative to max |y| for p_m; separately for the first 2 D rows and the rest.  The reference's error comes from the fixture's
``ref_vs_exact`` or, where there is no fixture, from the float64 row loop (regression_seq_oracle.row_loop) on the same input.
Every test prints worst error / tolerance; the measured figures are in profiles/regseq.md.
"""
import numpy as np
import pytest
import torch

import regression_oracle as orc
import regression_seq_oracle as seq
from conftest import load_golden

pytestmark = pytest.mark.gpu

B = seq.BLOCK
NS = (1, B - 1, B, B + 1, 3 * B + 17)
DEFAULT, dev, linreg, autoreg, hn_equal, synth, sweep = (seq.DEFAULT, seq.dev, seq.linreg, seq.autoreg, seq.hn_equal, seq.synth,
                                                         seq.sweep)


@pytest.mark.parametrize("name", seq.FIXTURES)
def test_fixtures(name):
    """Every fixture through the model on the GPU, at the bound of the module docstring.  Measured on one MI355X: worst
    error / tolerance 0.04 to 0.56 over the 18 fixtures (profiles/regseq.md)."""
    g = load_golden(name)
    w, y, start, exact, ref = seq.fixture_parts(g)
    m, args = seq.model_of(g, start, real=True)
    pred, nats = m.pred_and_update_sequence(*args, code_length=True)
    assert np.array_equal(pred, m.p_ms)
    print("worst error / tolerance: %.2f" % seq.check(name, (m.p_ms, m.p_lambdas, m.p_nus, nats), exact, ref, y, w.shape[1]))
    u, _ = seq.model_of(g, start, real=True)
    assert hn_equal(m, u.update_posterior(*args))
    if "p" in g:
        assert (m.p_m, m.p_lambda, m.p_nu) == (m.p_ms[-1], m.p_lambdas[-1], m.p_nus[-1])


@pytest.mark.parametrize("D", (1, 2, 15, 16, 17, 33, 128, 256))
def test_linreg_shapes(D):
    ns = NS if D < 128 else NS[:4]
    x, y = synth(D, max(ns), 300 + D)
    sweep(f"D = {D}", lambda: linreg(D), lambda n: (x[:n], y[:n]), ns, x, y, DEFAULT(D))


@pytest.mark.parametrize("padding", (None, "zeros"))
@pytest.mark.parametrize("p", (0, 1, 15, 16))
def test_ar_shapes(p, padding):
    rng = np.random.default_rng(400 + p)
    x = 0.3 + rng.standard_normal(3 * B + 17 + p)
    for t in range(1, len(x)):
        x[t] += 0.5 * x[t - 1]
    w, y = orc.lag_matrix(x, p, padding)
    t0 = 0 if padding == "zeros" else p
    ns = tuple(n for n in NS if n + t0 > p)                     # (the AR length rule: more than p values)
    sweep(f"AR({p}) padding = {padding}", lambda: autoreg(p), lambda n: (x[:n + t0], padding), ns, w, y, DEFAULT(p + 1))


@pytest.mark.parametrize("case", ("diffuse", "offset"))
def test_hard_priors_and_targets(case):
    """A diffuse prior (Lambda_0 = 1e-6 I: what the leading ramp is for) and targets around 100 (the cancellation in
    hn_beta)."""
    D, n = 8, 3 * B + 17
    x, y = synth(D, n, 500, intercept=100.0 if case == "offset" else 0.0)
    start = (np.zeros(D), np.eye(D) * (1e-6 if case == "diffuse" else 1.0), 1.0, 1.0)
    sweep(case, lambda: linreg(D, start), lambda k: (x[:k], y[:k]), (n,), x, y, start)


budget_for = seq.budget_for


@pytest.mark.parametrize("kind", ("linreg", "ar"))
def test_passes_are_bit_equal_to_one_call(kind):
    """chunk_bytes for 1 and for 3 blocks per pass against the default, and explicit regseq_pass calls on the same pieces."""
    from bayesml_amd import _regseq
    D, n = 5, 3 * B + 17
    x, y = synth(D, n + D, 600)
    make, args = (lambda: linreg(D), (x[:n], y[:n])) if kind == "linreg" else (lambda: autoreg(D - 1), (y[:n + D - 1],))
    one = make()
    base = one.pred_and_update_sequence(*args, code_length=True)
    assert one._seq_engine.passes == 1
    for blocks in (1, 3):
        m = make()
        got = m.pred_and_update_sequence(*args, code_length=True, chunk_bytes=budget_for(D, blocks))
        assert m._seq_engine.passes == -(-_regseq.block_count(n) // blocks) > 1
        assert all(np.array_equal(a, b) for a, b in zip(got, base)) and np.array_equal(m.p_lambdas, one.p_lambdas)
        assert hn_equal(m, one)
    if kind == "ar":
        return
    lib, d = _regseq.load_library(), dev()
    xd, yd = torch.from_numpy(x[:n]).to(d), torch.from_numpy(y[:n]).to(d)
    start = torch.from_numpy(_regseq.start_state(*DEFAULT(D))).to(d)
    carry = torch.zeros(D * D + D + 2, dtype=torch.float64, device=d)
    pm, pl, pn, nats = (torch.full((n,), np.nan, dtype=torch.float64, device=d) for _ in range(4))
    cuts = [0, 2, 3, 7, _regseq.block_count(n)]                  # passes of 2, 1, 4 blocks and the rest
    work = torch.empty(_regseq.work_slots(D, max(np.diff(cuts))), dtype=torch.float64, device=d)
    with torch.cuda.device(d):
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            r0, r1 = _regseq.block_start(n, b0), _regseq.block_start(n, b1)
            _regseq._check(lib.regseq_pass(D, 1, xd.data_ptr(), D, 1, yd.data_ptr(), n, r0, r1 - r0, start.data_ptr(),
                                           carry.data_ptr(), pm.data_ptr(), pl.data_ptr(), pn.data_ptr(), nats.data_ptr(),
                                           work.data_ptr(), _regseq.stream_ptr(d)), "regseq_pass")
    assert np.array_equal(pm.cpu().numpy(), base[0]) and np.array_equal(nats.cpu().numpy(), base[1])
    assert np.array_equal(pl.cpu().numpy(), one.p_lambdas) and np.array_equal(pn.cpu().numpy(), one.p_nus)
    stats = one._engine.stats(xd, yd).cpu().numpy()
    assert np.allclose(carry.cpu().numpy(), stats, rtol=1e-13, atol=1e-13) and carry[-1].item() == n


def test_dtypes_strides_and_offsets():
    """x and y in f32 / f64 independently, a row matrix with a row stride, four offsets into a series: device tensors are read
    where they lie, and the result is that of the widened contiguous copy, bit for bit."""
    D, n = 7, 2 * B + 5
    x, y = synth(D, n, 700)
    for xt in (np.float32, np.float64):
        for yt in (np.float32, np.float64):
            xs, ys = x.astype(xt), y.astype(yt)
            base = linreg(D).pred_and_update_sequence(xs.astype(np.float64), ys.astype(np.float64), code_length=True)
            wide = torch.zeros((n, D + 3), dtype=torch.from_numpy(xs).dtype, device=dev())
            wide[:, :D] = torch.from_numpy(xs)
            for xa in (xs, torch.from_numpy(xs).to(dev()), wide[:, :D]):
                m = linreg(D)
                got = m.pred_and_update_sequence(xa, ys if isinstance(xa, np.ndarray) else torch.from_numpy(ys).to(dev()),
                                                 code_length=True)
                assert all(isinstance(a, type(xa) if isinstance(xa, np.ndarray) else torch.Tensor) for a in got)
                assert all(np.array_equal(torch.as_tensor(a).cpu().numpy(), b) for a, b in zip(got, base))
                if not isinstance(xa, np.ndarray):
                    assert got[0].device == dev() and got[0].dtype == torch.float64
    series = (0.3 + np.random.default_rng(701).standard_normal(n + 8)).astype(np.float32)
    sd = torch.from_numpy(series).to(dev())
    for off in range(4):
        for padding in (None, "zeros"):
            base = autoreg(3).pred_and_update_sequence(series[off:].astype(np.float64), padding, code_length=True)
            got = autoreg(3).pred_and_update_sequence(sd[off:], padding, code_length=True)
            assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, base))


def test_two_runs_are_bit_equal():
    D, n = 40, 5 * B + 3
    x, y = synth(D, n, 800)
    a, b = linreg(D), linreg(D)
    ra = a.pred_and_update_sequence(x, y, code_length=True)
    rb = b.pred_and_update_sequence(x, y, code_length=True)
    assert all(np.array_equal(u, v) for u, v in zip(ra, rb)) and np.array_equal(a.p_lambdas, b.p_lambdas) and hn_equal(a, b)
    kl = linreg(D).pred_and_update_sequence(x, y, loss="KL")
    assert np.array_equal(kl.mean(), ra[0]) and np.array_equal(kl.kwds["df"], a.p_nus)


def test_a_long_sample_in_several_passes():
    """n = 200 003 at D = 16 with loss=None under an 8 MiB budget: finite code lengths whose sum is -log marginal
    likelihood of the end state, within 64 eps x the magnitudes summed on both sides."""
    from scipy.special import gammaln
    D, n = 16, 200003
    x, y, _ = orc.synth_linreg(D, n, 900, 2.0, np.float32)
    m = linreg(D)
    nats = m.pred_and_update_sequence(x, y, loss=None, code_length=True, chunk_bytes=8 << 20)
    assert m._seq_engine.passes > 1 and nats.shape == (n,) and np.all(np.isfinite(nats)) and m._n == n
    assert np.all(np.isfinite(m.p_ms)) and np.all(m.p_lambdas > 0) and m.p_nus[-1] == 2.0 + (n - 1)
    lml = m.calc_log_marginal_likelihood()
    terms = [m.hn_alpha * np.log(m.hn_beta), gammaln(m.hn_alpha), 0.5 * np.linalg.slogdet(m.hn_lambda_mat)[1],
             0.5 * n * np.log(2 * np.pi)]
    bound = 64 * seq.EPS * (np.abs(nats).sum() + np.abs(terms).sum())
    print(f"sum nats + lml = {nats.sum() + lml:.2e}, bound {bound:.2e}, passes {m._seq_engine.passes}")
    assert abs(nats.sum() + lml) <= bound
