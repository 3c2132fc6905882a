"""``pred_and_update_sequence`` of linearregression / autoregressive on the CPU: the NumPy restatement of the block form
(tests/regression_seq_oracle.py) against reference-generated fixtures, the schedule and the workspace plan, the C ABI of
include/regseq.h without a GPU, and the models' host logic through the ``_regseq_pass_factory`` seam.

Tolerance (regression_seq_oracle.check): an output is compared with the long-double loop and must lie within 8 x the
reference loop's own error on the same rows - from the fixture's ``ref_vs_exact``, separately for the first 2 D rows and for
the rest - and never below 64 eps; relative per row for p_lambda and nats (a code length's magnitude floored at 1), relative
to max |y| for p_m.  Measured here (worst error / tolerance, the restatement and the models on the stand-in alike): 0.53 on
the first 2 D rows of regression_seq_ar_p1_diffuse (p_m, 1.3e-11 / 2.5e-11), 0.14 and below on the other 17 fixtures.
"""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import regression_oracle as orc
import regression_seq_cases as cases
import regression_seq_oracle as seq
from conftest import ROOT, load_golden

B = seq.BLOCK
LOSSES = ("squared", "0-1", "abs", "KL", None)


stand_ins, model_of = seq.stand_ins, seq.model_of


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", seq.FIXTURES)
def test_block_form_against_the_reference_fixtures(name):
    g = load_golden(name)
    w, y, start, exact, ref = seq.fixture_parts(g)
    got = seq.block_form(w, y, seq.start_state(*start))
    print("worst error / tolerance: %.2f" % seq.check(name, got, exact, ref, y, w.shape[1]))


def test_no_fixture_block_is_flagged_by_its_data():
    """Past the first 2 D rows max_i K_ii of every fixture's blocks is far below the double-double threshold (measured:
    2.9 at most, regression_seq_linreg_d3_default), so the criterion leaves their bits alone."""
    worst = 0.0
    for name in seq.FIXTURES:
        w, y, start, _exact, _ref = seq.fixture_parts(load_golden(name))
        diag = []
        got = seq.block_form(w, y, seq.start_state(*start), diag=diag)
        worst = max([worst] + [k for _lo, _hi, head, k in diag if not head])
        for a, b in zip(got, seq.block_form(w, y, seq.start_state(*start), dd_threshold=None)):
            assert np.array_equal(a, b), name
    print(f"largest K_ii past the first 2 D rows: {worst:.2f}")
    assert worst <= seq.DD_THRESHOLD / 8


@pytest.mark.parametrize("name", cases.NAMES)
def test_block_form_on_late_features(name):
    """A regressor that switches on late (regression_seq_cases.py), at the bound of the module docstring against the
    float64 row loop.  Measured here, worst error / tolerance: late column 0.18, late dummy 0.16, control 0.09 (all on the
    first 2 D rows; 0.08 and below on the rest).  With the data out of the double-double decision the two diffuse cases
    miss the bound on the rest by factors of 1012 (p_m), 3004 (p_lambda), 1344 (nats) and 13464, 1416, 1400: the onset block
    [63, 127) has K_ii of 4.7e6 and 1.0e6, every other block past 2 D rows 2.1 at most; the control's has 5.7 and its bits
    do not depend on the criterion."""
    c = cases.make(name)
    assert c.onset_block == slice(63, 127) and not c.x[:c.onset, 3 if c.onset == 100 else 2].any()
    exact = seq.ld_row_loop(c.x, c.y, *c.start)
    ref = seq.row_loop(c.x, c.y, *c.start)[:4]
    diag = []
    got = seq.block_form(c.x, c.y, seq.start_state(*c.start), diag=diag)
    print("worst error / tolerance: %.2f" % seq.check(name, got, exact, ref, c.y, cases.D))
    flagged = [(lo, hi) for lo, hi, head, k in diag if not head and k > seq.DD_THRESHOLD]
    old = seq.block_form(c.x, c.y, seq.start_state(*c.start), dd_threshold=None)
    if name == "control":
        assert flagged == [] and all(np.array_equal(a, b) for a, b in zip(got, old))
        return
    assert flagged == [(63, 127)]
    with pytest.raises(AssertionError):
        seq.check(name + " (rows alone decide)", old, exact, ref, c.y, cases.D)
    rows = np.r_[0:63, 127:cases.N]
    assert all(np.array_equal(a[rows], b[rows]) for a, b in zip(got, old))       # (the other blocks keep their bits)


@pytest.mark.parametrize("per_pass", (1, 2, 7))
def test_block_form_in_passes_is_bit_equal_to_one_pass(per_pass):
    rng = np.random.default_rng(per_pass)
    w, y = rng.standard_normal((3 * B + 17, 5)), rng.standard_normal(3 * B + 17)
    start = seq.start_state(np.zeros(5), np.eye(5), 1.0, 1.0)
    for a, b in zip(seq.block_form(w, y, start), seq.block_form(w, y, start, blocks_per_pass=per_pass)):
        assert np.array_equal(a, b)


# ---- the schedule, the plan, the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, B - 1, B, B + 1, 3 * B + 17))
def test_schedule(n):
    """Lengths 1, 2, ..., B / 2, B, ..., a tail, summing to n: the oracle's construction, the binding's arithmetic and the
    library agree."""
    from bayesml_amd import _regseq
    lib = _regseq.load_library()
    bounds = seq.schedule(n)
    lengths = np.diff(bounds)
    want = [1 << k for k in range(B.bit_length() - 1)] + [B] * (n // B + 1)
    assert bounds[0] == 0 and bounds[-1] == n and lengths.sum() == n and lengths.min() >= 1
    assert list(lengths[:-1]) == want[:len(lengths) - 1] and lengths[-1] <= want[len(lengths) - 1]
    count = len(bounds) - 1
    assert _regseq.block_count(n) == count == lib.regseq_block_count(n)
    assert [_regseq.block_start(n, b) for b in range(count + 1)] == bounds
    assert [lib.regseq_block_start(n, b) for b in range(count + 1)] == bounds
    assert lib.regseq_block_start(n, count + 1) == -1 and lib.regseq_block_start(n, -1) == -1


def test_plan_and_work_len_agree():
    from bayesml_amd import _regseq
    lib = _regseq.load_library()
    assert _regseq.BLOCK == B
    for D in (1, 16, 17, 33, 128, 255, 256):
        assert lib.regseq_block(D) == B
        for blocks in (1, 2, 1000):
            assert _regseq.work_slots(D, blocks) == lib.regseq_work_len(D, blocks)
        for budget in (1 << 20, 8 << 20, None):
            nb = _regseq.plan_blocks(10 ** 6, D, budget)
            limit = _regseq.DEFAULT_CHUNK_BYTES if budget is None else budget
            assert nb >= 1 and (nb == 1 or 8 * _regseq.work_slots(D, nb) <= limit)
            assert nb == _regseq.block_count(10 ** 6) or 8 * _regseq.work_slots(D, nb + 1) > limit
        assert _regseq.plan_blocks(5, D) == _regseq.block_count(5) == 3
    assert lib.regseq_block(0) == -1 and lib.regseq_block(257) == -1 and lib.regseq_block_count(0) == -1
    assert lib.regseq_work_len(0, 1) == -1 and lib.regseq_work_len(257, 1) == -1 and lib.regseq_work_len(4, 0) == -1


def test_header_library_and_ctypes_table_agree():
    import re
    from bayesml_amd import _regseq
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/regseq.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(regseq_[a-z0-9_]+)\s*\(", text)))
    lib = _regseq.load_library()
    assert sorted(_regseq.SYMBOLS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.regseq_abi_version() == 1 == int(re.search(r"#define REGSEQ_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"#define REGSEQ_BLOCK (\d+)", text).group(1)) == B
    assert "regseq_" not in open(ROOT + "/include/regvb.h").read()


def test_argument_errors_without_a_gpu():
    from bayesml_amd import _regseq
    lib = _regseq.load_library()
    P, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)          # never dereferenced

    def matrix(D=4, xt=0, x=P, ldx=4, yt=0, y=P, n=200, begin=0, count=200, start=P, carry=P, pm=P, pl=None, pn=None,
               nats=None, work=P):
        return lib.regseq_pass(D, xt, x, ldx, yt, y, n, begin, count, start, carry, pm, pl, pn, nats, work, None)

    def window(p=3, xt=1, x=P, length=203, pad=0, begin=0, count=200, start=P, carry=P, pm=None, pl=None, pn=None, nats=P,
               work=P):
        return lib.regseq_pass_window(p, xt, x, length, pad, begin, count, start, carry, pm, pl, pn, nats, work, None)

    def refused(rc, code, text):
        assert rc == code and text in lib.regseq_last_error().decode(), (rc, lib.regseq_last_error())

    refused(matrix(D=0), 1, "D must be >= 1")
    refused(matrix(D=257, ldx=257), 2, "D > 256 is not supported")
    refused(window(p=256, length=600), 2, "p + 1 > 256")
    refused(window(p=-1), 1, "p must be >= 0")
    refused(matrix(xt=2), 1, "x_dtype")
    refused(matrix(yt=5), 1, "y_dtype")
    refused(window(pad=2), 1, "padding")
    refused(window(length=3), 1, "length must be > p")
    refused(matrix(n=0), 1, "n_rows")
    refused(matrix(ldx=3), 1, "ldx")
    for null in ("x", "y", "start", "carry", "work"):
        refused(matrix(**{null: None}), 1, "null pointer")
    for null in ("x", "start", "carry", "work"):
        refused(window(**{null: None}), 1, "null pointer")
    refused(matrix(xt=1, x=odd), 1, "aligned")
    refused(matrix(y=ctypes.c_void_p(4098)), 1, "aligned")
    refused(window(x=odd), 1, "aligned")
    for name in ("start", "carry", "work", "pm", "nats"):
        refused(matrix(**{name: odd}), 1, "8-byte aligned")
    # a range that is not whole blocks of the schedule of 200 rows (blocks start at 0, 1, 3, ..., 63, 127, 191)
    refused(matrix(begin=2, count=198), 1, "not whole blocks")
    refused(matrix(begin=0, count=100), 1, "not whole blocks")
    refused(matrix(begin=64, count=63), 1, "not whole blocks")
    refused(matrix(begin=63, count=138), 1, "not whole blocks")
    refused(window(begin=127, count=0), 1, "row_count")
    refused(window(begin=-1, count=2), 1, "not whole blocks")


# ---- the models on the stand-in -------------------------------------------------------------------------------------------
def loop_of(g, start):
    """(p_ms, p_lambdas, p_nus) of the models' own per-row loop on the stand-in, and the model afterwards."""
    m, args = model_of(g, start)
    out = ([], [], [])
    if "p" in g:
        p, x = int(g["p"]), g["x"]
        for t in range(p, len(x)):
            m.pred_and_update(x[t - p:t + 1])
            for o, v in zip(out, (m.p_m, m.p_lambda, m.p_nu)):
                o.append(float(v))
    else:
        for xi, yi in zip(g["x"], g["y"]):
            m.calc_pred_dist(xi)
            for o, v in zip(out, (m.p_ms, m.p_lambdas, m.p_nus)):
                o.append(float(v[0]))
            m.update_posterior(xi, yi)
    return [np.array(o) for o in out], m


@pytest.mark.parametrize("name", seq.FIXTURES)
def test_models_on_the_stand_in(name):
    """The sequence equals the loop (at the fixture's tolerance, against the long-double loop), hn_* are the bits of
    update_posterior, the p_* attributes hold the traces, and sum nats = -log marginal likelihood of the end state within
    64 eps x the magnitudes summed on both sides.  The last is not asked of the diffuse-prior fixtures: their first 2 D code
    lengths are conditioned like Lambda (1e6 and more) in any float64 evaluation - the reference loop's own are 1e-10
    from the long-double values (``ref_vs_exact``), beyond that bound - and the per-row comparison above is their check."""
    g = load_golden(name)
    w, y, start, exact, ref = seq.fixture_parts(g)
    D, n = w.shape[1], len(y)
    m, args = model_of(g, start)
    pred, nats = m.pred_and_update_sequence(*args, code_length=True)
    assert isinstance(pred, np.ndarray) and pred.dtype == np.float64 and pred.shape == nats.shape == (n,)
    got = (m.p_ms, m.p_lambdas, m.p_nus, nats)
    assert np.array_equal(pred, m.p_ms) and all(a.shape == (n,) for a in got)
    print("worst error / tolerance: %.2f" % seq.check(name, got, exact, ref, y, D))
    # the loop of the same models: what the sequence replaces
    loop, lm = loop_of(g, start)
    seq.check(name + " (the models' loop)", (*loop, nats), exact, ref, y, D)
    u, _ = model_of(g, start)
    u.update_posterior(*args)
    for k in ("hn_mu_vec", "hn_lambda_mat", "hn_alpha", "hn_beta"):
        assert np.array_equal(getattr(m, k), getattr(u, k)), k
        assert np.allclose(getattr(m, k), g[k], rtol=1e-6, atol=1e-9), k
    if "p" in g:
        assert (m.p_m, m.p_lambda, m.p_nu) == (m.p_ms[-1], m.p_lambdas[-1], m.p_nus[-1])
    else:
        assert m._n == u._n == n
    if "diffuse" in name:
        return
    lml = orc.log_marginal_likelihood(start[1], start[2], start[3], m.hn_lambda_mat, m.hn_alpha, m.hn_beta, n)
    from scipy.special import gammaln
    terms = [start[2] * np.log(start[3]), m.hn_alpha * np.log(m.hn_beta), gammaln(m.hn_alpha), gammaln(start[2]),
             0.5 * np.linalg.slogdet(start[1])[1], 0.5 * np.linalg.slogdet(m.hn_lambda_mat)[1], 0.5 * n * np.log(2 * np.pi)]
    bound = 64 * seq.EPS * (np.abs(nats).sum() + np.abs(terms).sum())
    print(f"sum nats + lml = {nats.sum() + lml:.2e}, bound {bound:.2e}")
    assert abs(nats.sum() + lml) <= bound


def small_case(kind, as_torch, dtype):
    from bayesml_amd import autoregressive as ar, linearregression as lr
    rng = np.random.default_rng(7)
    if kind == "ar":
        m, args = stand_ins(ar.LearnModel(2)), (rng.standard_normal(40).astype(dtype),)
        n = 38
    else:
        x = rng.standard_normal((40, 3)).astype(dtype)
        m, args = stand_ins(lr.LearnModel(3)), (x, (x @ np.ones(3) + rng.standard_normal(40)).astype(dtype))
        n = 40
    if as_torch:
        args = tuple(torch.from_numpy(a) for a in args)
    return m, args, n


@pytest.mark.parametrize("kind", ("linreg", "ar"))
@pytest.mark.parametrize("as_torch", (False, True))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_return_types_for_every_loss(kind, as_torch, dtype):
    from bayesml_amd._exceptions import CriteriaError
    want = torch.Tensor if as_torch else np.ndarray
    base = None
    for loss in LOSSES:
        for code_length in (False, True):
            m, args, n = small_case(kind, as_torch, dtype)
            kw = dict(loss=loss, code_length=code_length)
            if loss is None and not code_length:
                with pytest.raises(CriteriaError):
                    m.pred_and_update_sequence(*args, **kw)
                continue
            out = m.pred_and_update_sequence(*args, **kw)
            pred, nats = out if (code_length and loss is not None) else ((None, out) if loss is None else (out, None))
            if loss is not None and code_length:
                assert isinstance(out, tuple) and len(out) == 2
            if nats is not None:
                assert isinstance(nats, want) and tuple(nats.shape) == (n,) and nats.dtype in (np.float64, torch.float64)
            if loss == "KL":
                assert type(pred).__name__ == "rv_continuous_frozen" or hasattr(pred, "logpdf")
                assert np.array_equal(pred.mean(), m.p_ms) and np.array_equal(pred.kwds["df"], m.p_nus)
            elif loss is not None:
                assert isinstance(pred, want) and tuple(pred.shape) == (n,) and pred.dtype in (np.float64, torch.float64)
                assert np.array_equal(np.asarray(pred), m.p_ms)
            assert isinstance(m.p_ms, np.ndarray) and m.p_ms.shape == m.p_lambdas.shape == m.p_nus.shape == (n,)
            if base is None:
                base = (m.p_ms.copy(), m.p_lambdas.copy(), m.hn_mu_vec.copy(), m.hn_beta)
            assert np.array_equal(m.p_ms, base[0]) and np.array_equal(m.p_lambdas, base[1])
            assert np.array_equal(m.hn_mu_vec, base[2]) and m.hn_beta == base[3]
    m, args, _ = small_case(kind, as_torch, dtype)
    for bad in ("l2", 0, "kl"):
        with pytest.raises(CriteriaError, match="Unsupported loss function"):
            m.pred_and_update_sequence(*args, loss=bad)


def test_padding_and_the_ar_length_rule():
    from bayesml_amd import autoregressive as ar
    from bayesml_amd._exceptions import DataFormatError
    x = np.random.default_rng(3).standard_normal(30)
    for padding, n in ((None, 27), ("zeros", 30), ("anything else", 27)):
        m = stand_ins(ar.LearnModel(3))
        pm = m.pred_and_update_sequence(x, padding)
        u = stand_ins(ar.LearnModel(3)).update_posterior(x, padding)
        assert pm.shape == (n,) and np.array_equal(m.hn_mu_vec, u.hn_mu_vec) and m.hn_beta == u.hn_beta
        w, y = orc.lag_matrix(x, 3, padding)
        want = seq.block_form(w, y, seq.start_state(np.zeros(4), np.eye(4), 1.0, 1.0))
        assert np.array_equal(pm, want[0]) and np.array_equal(m.p_lambdas, want[1]) and np.array_equal(m.p_nus, want[2])
    m = stand_ins(ar.LearnModel(3))
    with pytest.raises(DataFormatError):
        m.pred_and_update_sequence(x[:3])
    with pytest.raises(DataFormatError):
        m.pred_and_update_sequence(x[:3], "zeros")


def test_a_refused_sample_changes_nothing():
    from bayesml_amd import autoregressive as ar, linearregression as lr
    from bayesml_amd._exceptions import CriteriaError, DataFormatError
    x = np.random.default_rng(4).standard_normal((12, 3))
    for m, calls in ((stand_ins(lr.LearnModel(3)), [(x[:, :2], x[:, 0]), (x, x[:5, 0]), (x, "y"), ("x", 1.0)]),
                     (stand_ins(ar.LearnModel(3)), [(x,), (x[:3, 0],), ("abc",), (torch.ones(9, dtype=torch.int64),)])):
        m.pred_and_update_sequence(*((x, x[:, 0]) if len(calls[0]) == 2 else (x[:, 0],)))
        before = pickle.dumps(m)
        for args in calls:
            with pytest.raises(DataFormatError):
                m.pred_and_update_sequence(*args)
        with pytest.raises(CriteriaError):
            m.pred_and_update_sequence(*((x, x[:, 0]) if len(calls[0]) == 2 else (x[:, 0],)), loss="cubic")
        assert pickle.dumps(m) == before


def test_no_rows_is_no_work():
    from bayesml_amd import linearregression as lr
    m = stand_ins(lr.LearnModel(3))
    pred, nats = m.pred_and_update_sequence(np.zeros((0, 3)), np.zeros(0), code_length=True)
    assert pred.shape == nats.shape == m.p_lambdas.shape == m.p_nus.shape == (0,) and m.hn_alpha == 1.0 and m._n == 0


def test_dtypes_reach_the_engine_unchanged():
    from bayesml_amd import linearregression as lr
    seen = []

    def recording(D):
        eng = seq.CpuRegressionSeqPass(D)
        seen.append(eng)
        return eng
    rng = np.random.default_rng(5)
    for xt, yt in ((np.float32, np.float64), (np.float64, np.float32)):
        m = stand_ins(lr.LearnModel(2))
        m._regseq_pass_factory = recording
        m.pred_and_update_sequence(rng.standard_normal((9, 2)).astype(xt), rng.standard_normal(9).astype(yt))
        assert seen[-1].last_dtypes == (int(xt is np.float64), int(yt is np.float64))


@pytest.mark.parametrize("kind", ("linreg", "ar"))
def test_pickle_round_trip(kind):
    m, args, n = small_case(kind, True, np.float64)
    m.pred_and_update_sequence(*args)
    m._seq_engine = object()                    # whatever the engine is, it does not travel
    m._regseq_pass_factory = None
    m._reg_pass_factory = None
    c = pickle.loads(pickle.dumps(m))
    assert c._seq_engine is None and c._engine is None
    assert np.array_equal(c.p_ms, m.p_ms) and np.array_equal(c.p_lambdas, m.p_lambdas) and np.array_equal(c.p_nus, m.p_nus)
    assert np.array_equal(c.hn_lambda_mat, m.hn_lambda_mat) and c.hn_beta == m.hn_beta and c.p_ms.shape == (n,)


def test_product_path_fails_loudly_without_a_gpu():
    if torch.cuda.is_available():
        return                                  # (an unmarked test does not touch the device)
    from bayesml_amd import autoregressive as ar, linearregression as lr
    from bayesml_amd._engine import EngineUnavailableError
    with pytest.raises(EngineUnavailableError):
        lr.LearnModel(2).pred_and_update_sequence(np.zeros((4, 2)), np.zeros(4))
    m = ar.LearnModel(1)
    with pytest.raises(EngineUnavailableError):
        m.pred_and_update_sequence(np.zeros(4))
    assert m.hn_alpha == 1.0
