"""The sequential regression kernels (csrc/regseq_kernels.h) on the GPU at the edges of their branches: every length of the
cut last block in both K paths, every slice count of the binary64 K path, lag windows across 16-column slices, a second call
on a model, passes over padded windows and strided rows, the ends of the code length's ranges, and regressors that switch on
late under a diffuse prior (regression_seq_cases.py).

Oracle and bound are those of test_gpu_regression_seq.py (regression_seq_oracle.check): the long-double row loop, 8 x the
float64 row loop's own error on the same rows and never below 64 eps, separately for the first 2 D rows and the rest.  Every
test prints worst error / tolerance; the measured figures are in profiles/regseq.md.
"""
import numpy as np
import pytest
import torch

import regression_oracle as orc
import regression_seq_cases as cases
import regression_seq_oracle as seq

pytestmark = pytest.mark.gpu

B = seq.BLOCK
CUTS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)       # the waves of a block hold 16 rows each
DIFFUSE = lambda D: (np.zeros(D), np.eye(D) * 1e-6, 1.0, 1.0)      # noqa: E731


def correlated(D, seed):
    """The "posterior" prior of tests/golden/make_golden_regression_seq.py as a start state."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((D, D))
    return rng.standard_normal(D) * 0.3, np.eye(D) * 2.0 + a @ a.T / D, 2.5, 0.75


# ---- the cut last block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 40))
def test_every_cut(D):
    """Calls on the first n rows of one sample for every n up to 66 (each ramp block as the cut block; no row, one row and
    two rows in the first block of 64) and for 63 + L rows, L around every multiple of 16.  The block at row 63 starts past
    2 D rows at D = 3 (binary64 K on the matrix pipe) and within them at D = 40 (double-double)."""
    ns = tuple(range(1, B + 3)) + tuple(B - 1 + L for L in CUTS)
    x, y = seq.synth(D, 130, 1000 + D)
    seq.sweep(f"D = {D}", lambda: seq.linreg(D), lambda n: (x[:n], y[:n]), ns, x, y, seq.DEFAULT(D))


@pytest.mark.parametrize("L", CUTS)
def test_rows_past_the_end_write_nothing(L):
    """regseq_pass itself on 63 + L rows at D = 3, the four outputs 64 elements longer than the sample and filled with NaN:
    the tail is still NaN afterwards and the rows are the model's, bit for bit."""
    from bayesml_amd import _regseq
    D, n = 3, B - 1 + L
    x, y = seq.synth(D, 130, 1000 + D)
    m = seq.linreg(D)
    base = m.pred_and_update_sequence(x[:n], y[:n], code_length=True)
    lib, d = _regseq.load_library(), seq.dev()
    xd, yd = torch.from_numpy(x[:n]).to(d), torch.from_numpy(y[:n]).to(d)
    start = torch.from_numpy(_regseq.start_state(*seq.DEFAULT(D))).to(d)
    carry = torch.zeros(D * D + D + 2, dtype=torch.float64, device=d)
    outs = [torch.full((n + B,), np.nan, dtype=torch.float64, device=d) for _ in range(4)]
    work = torch.empty(_regseq.work_slots(D, _regseq.block_count(n)), dtype=torch.float64, device=d)
    with torch.cuda.device(d):
        _regseq._check(lib.regseq_pass(D, 1, xd.data_ptr(), D, 1, yd.data_ptr(), n, 0, n, start.data_ptr(), carry.data_ptr(),
                                       *(o.data_ptr() for o in outs), work.data_ptr(), _regseq.stream_ptr(d)), "regseq_pass")
    pm, pl, pn, nats = (o.cpu().numpy() for o in outs)
    assert all(np.all(np.isnan(o[n:])) for o in (pm, pl, pn, nats))
    assert np.array_equal(pm[:n], base[0]) and np.array_equal(nats[:n], base[1])
    assert np.array_equal(pl[:n], m.p_lambdas) and np.array_equal(pn[:n], m.p_nus)


# ---- the slices of the binary64 K path ---------------------------------------------------------------------------------------
SLICES = [(D, prior) for D in (49, 64, 65, 128, 256) for prior in ("default", "diffuse")] + [(64, "correlated"), (128, "correlated")]


@pytest.mark.parametrize("D,prior", SLICES)
def test_every_slice_count(D, prior):
    """nt = 4, 4, 5, 8, 16 slices of sixteen columns with K accumulated on the matrix pipe: the sample reaches one whole block
    and a cut one of 17 rows past the first block that starts at or after 2 D rows.  At D = 64 and 128 (D a multiple of 16:
    no padding between the factor and the tail of the state area) also from a correlated Lambda_0 with mu_0 != 0.  At
    D = 256 the long-double loop factorises only at the first 40 rows, around row 2 D and from row 575 on."""
    first = next(b for b in seq.schedule(4 * D + 2 * B) if b >= 2 * D)
    assert first == {49: 127, 64: 191, 65: 191, 128: 319, 256: 575}[D]
    n = first + B + 17
    x, y = seq.synth(D, n, 1100 + D)
    start = {"default": seq.DEFAULT, "diffuse": DIFFUSE, "correlated": lambda k: correlated(k, 1200 + k)}[prior](D)
    rows = None if D < 256 else [*range(40), *range(2 * D - 8, 2 * D + 9), *range(first, n)]
    seq.sweep(f"D = {D} {prior}", lambda: seq.linreg(D, start), lambda k: (x[:k], y[:k]), (n,), x, y, start, rows=rows)


# ---- lag windows across slices -----------------------------------------------------------------------------------------------
def ar_series(p, dtype=np.float64):
    rng = np.random.default_rng(1300 + p)
    x = 0.3 + rng.standard_normal(3 * B + 17 + p)
    for t in range(1, len(x)):
        x[t] += 0.5 * x[t - 1]
    return x.astype(dtype)


@pytest.mark.parametrize("padding", (None, "zeros"))
@pytest.mark.parametrize("p", (17, 31, 32, 63))
def test_ar_degrees_across_slices(p, padding):
    """p + 1 = 18, 32, 33, 64 window columns: the window source is read across two, three and four slices."""
    x = ar_series(p)
    w, y = orc.lag_matrix(x, p, padding)
    t0 = 0 if padding == "zeros" else p
    seq.sweep(f"AR({p}) padding = {padding}", lambda: seq.autoreg(p), lambda n: (x[:n + t0], padding), (3 * B + 17,), w, y,
              seq.DEFAULT(p + 1))


def test_ar_across_slices_in_f32():
    p = 32
    x = ar_series(p, np.float32)
    w, y = orc.lag_matrix(x.astype(np.float64), p, None)
    seq.sweep(f"AR({p}) f32", lambda: seq.autoreg(p), lambda n: (x[:n + p], None), (3 * B + 17,), w, y, seq.DEFAULT(p + 1))


# ---- a second call on a model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", (1, 5, 100))
def test_second_call(n1):
    """Rows [0, n1) and [n1, n) in two calls from a diffuse prior: after 1 and after 5 rows the second call's ramp and first
    2 D rows start from a posterior that is still singular to working precision.  The oracle starts from the model's own
    hn_* after the first call; hn_* after both are update_posterior's on the two pieces."""
    D, n = 8, 3 * B + 17
    x, y = seq.synth(D, n, 1400)
    m = seq.linreg(D, DIFFUSE(D))
    m.pred_and_update_sequence(x[:n1], y[:n1])
    start = tuple(np.copy(getattr(m, k)) for k in seq.HN)
    w2, y2 = x[n1:], y[n1:]
    pred, nats = m.pred_and_update_sequence(w2, y2, code_length=True)
    exact, ref = seq.ld_row_loop(w2, y2, *start), seq.row_loop(w2, y2, *start)[:4]
    worst = seq.check(f"second call after {n1} rows", (pred, m.p_lambdas, m.p_nus, nats), exact, ref, y2, D)
    print(f"second call after {n1} rows: worst error / tolerance {worst:.2f}")
    u = seq.linreg(D, DIFFUSE(D))
    u.update_posterior(x[:n1], y[:n1])
    assert seq.hn_equal(m, u.update_posterior(w2, y2))


# ---- passes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("ar zeros", "strided f32"))
def test_passes_are_bit_equal_to_one_call(kind):
    """Passes of 1 and of 3 blocks against one pass: AR(4) windows with zero padding, and D = 33 on f32 rows that lie
    in a wider device matrix."""
    from bayesml_amd import _regseq
    n = 3 * B + 17
    if kind == "ar zeros":
        D = 5
        make, args = (lambda: seq.autoreg(D - 1)), (ar_series(D - 1)[:n], "zeros")
    else:
        D = 33
        x, y = seq.synth(D, n, 1500)
        wide = torch.zeros((n, D + 3), dtype=torch.float32, device=seq.dev())
        wide[:, :D] = torch.from_numpy(x.astype(np.float32))
        make, args = (lambda: seq.linreg(D)), (wide[:, :D], torch.from_numpy(y).to(seq.dev()))
        assert args[0].stride(0) == D + 3
    host = lambda out: [torch.as_tensor(a).cpu().numpy() for a in out]      # noqa: E731
    one = make()
    base = host(one.pred_and_update_sequence(*args, code_length=True))
    assert one._seq_engine.passes == 1
    for blocks in (1, 3):
        m = make()
        got = host(m.pred_and_update_sequence(*args, code_length=True, chunk_bytes=seq.budget_for(D, blocks)))
        assert m._seq_engine.passes == -(-_regseq.block_count(n) // blocks) > 1
        assert all(np.array_equal(a, b) for a, b in zip(got, base)) and np.array_equal(m.p_lambdas, one.p_lambdas)
        assert seq.hn_equal(m, one)


# ---- the ends of the code length's ranges ------------------------------------------------------------------------------------
def code_length_case(case):
    D, n = 8, 3 * B + 17
    x, y, theta = orc.synth_linreg(D, n, 1600, 2.0, np.float64)
    start = seq.DEFAULT(D)
    if case in ("alpha 63.25", "alpha 63.5"):           # alpha_i = alpha_0 + i / 2 passes 64 (at 63.5: is 64 exactly at row 1)
        start = (np.zeros(D), np.eye(D), float(case.split()[1]), 40.0)
    elif case == "alpha = beta = 1e6":
        start = (np.zeros(D), np.eye(D), 1e6, 1e6)
    elif case == "y 1e-6":
        y = y * 1e-6
    elif case == "y 1e6":
        y = y * 1e6
    elif case == "noise-free":
        y = x @ theta
    elif case == "zero and repeated rows":
        x = x.copy()
        x[5] = x[64] = 0.0
        x[100:110] = x[99]
    return x, y, start


@pytest.mark.parametrize("case", ("alpha 63.25", "alpha 63.5", "alpha = beta = 1e6", "y 1e-6", "y 1e6", "noise-free",
                                  "zero and repeated rows"))
def test_code_length_edges(case):
    x, y, start = code_length_case(case)
    D = x.shape[1]
    seq.sweep(case, lambda: seq.linreg(D, start), lambda k: (x[:k], y[:k]), (len(y),), x, y, start)


# ---- regressors that switch on late --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_late_features(name):
    """The onset block [63, 127) of the two diffuse cases has K_ii of 1e6 past the first 2 D rows: its K must come from
    double-double (kDdThreshold); the control's has 5.7 and stays on the matrix pipe."""
    c = cases.make(name)
    seq.sweep(name, lambda: seq.linreg(cases.D, c.start), lambda k: (c.x[:k], c.y[:k]), (cases.N,), c.x, c.y, c.start)
