"""``pred_and_update_sequence`` of the five scalar conjugate models on the device (include/expseq.h): the checks of
tests/test_expfam_seq.py on the real pass, at every tile and scan edge.  T is the tile length and W the scan workgroup; the
edge lengths are 1, 2, T - 1, T, T + 1, 3 T + 17 and W T + 3 T + 17 (more tiles than scan threads)."""
import warnings

import numpy as np
import pytest
import torch

import expfam_seq_oracle as orc
from conftest import load_golden
from expfam_seq_oracle import T, same_bits

from bayesml_amd import _expseq as xs
from bayesml_amd._exceptions import DataFormatError, ResultWarning

pytestmark = pytest.mark.gpu
BIG = orc.EDGE_LENGTHS[-1]
DEGREES = [(1, 3 * T + 17), (2, 3 * T + 17), (5, 3 * T + 17), (64, 3 * T + 17), (65, 3 * T + 17), (300, 3 * T + 17),
           (4096, T + 1)]


# ---- 1. the reference's fixtures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(orc.FIXTURES))
def test_reference_fixture(name):
    orc.check_fixture(name, load_golden(f"expfam_seq_{name}.npz"), None)


@pytest.mark.parametrize("degree", [3, 300])
def test_reference_fixture_categorical(degree):
    orc.check_categorical_fixture(degree, load_golden(f"expfam_seq_categorical_d{degree}.npz"), None)


# ---- 2. integer state is exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", orc.EDGE_LENGTHS)
@pytest.mark.parametrize("family", [xs.BERNOULLI, xs.POISSON])
def test_integer_state_is_exact(family, n):
    """Past 3 T + 17 the per-value loop would take many seconds: there the loop's value is the one-rounding form on NumPy's
    exact integer prefix sums (equal to the loop for a dyadic start), and hn_* are update_posterior's."""
    orc.check_integer_state(family, n, None, with_loop=n < BIG)


@pytest.mark.parametrize("n", orc.EDGE_LENGTHS)
def test_categorical_integer_state_is_exact(n):
    orc.check_categorical_integer_state(3, n, None, with_loop=n < BIG)
    if n >= T:
        orc.check_categorical_integer_state(5, n, None, kind="edges", with_loop=False)


# ---- 3. float state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", orc.EDGE_LENGTHS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_state_within_the_derived_bounds(dtype, n):
    orc.check_float_state(xs.EXPONENTIAL, n, dtype, None, None)
    for recipe in ("std", "tight", "offset"):
        orc.check_float_state(xs.NORMAL, n, dtype, recipe, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_state_against_the_loop(dtype):
    orc.check_against_loop(xs.EXPONENTIAL, dtype, None, None)
    for recipe in ("std", "tight", "offset"):
        orc.check_against_loop(xs.NORMAL, dtype, recipe, None)


# ---- 4. code lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [T + 1, BIG])
def test_code_lengths_within_their_bounds(n):
    for family, start in ((xs.BERNOULLI, (0.5, 0.5)), (xs.POISSON, (1.0, 1.0)), (xs.EXPONENTIAL, (1.0, 1.0)),
                          (xs.NORMAL, (0.0, 1.0, 1.0, 1.0))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ResultWarning)
            print("family", family, "n", n, "worst error / bound", orc.check_nats(family, orc.sample(family, n, seed=3), start, None))
    for family, start in orc.LONG_START.items():
        print("family", family, "n", n, "long posterior", orc.check_nats(family, orc.sample(family, n, seed=4), start, None))


@pytest.mark.parametrize("degree, n", [(1, T + 1), (5, 3 * T + 17), (300, 3 * T + 17), (4096, T + 1), (3, BIG)])
def test_categorical_code_lengths(degree, n):
    print("categorical", degree, n, "worst error / bound", orc.check_categorical_nats(degree, n, None))
    if degree == 5:
        long_alpha = 2e6 + 0.3 + 0.7 * np.sqrt(np.arange(1, degree + 1))          # as after 1e7 earlier values
        print("categorical long posterior", orc.check_categorical_nats(degree, n, None, alpha=long_alpha))


# ---- 5. categorical rows and chunks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree, n", DEGREES)
def test_categorical_rows_argmax_and_chunks(degree, n):
    orc.check_categorical_rows_and_chunks(degree, n, None)


def test_categorical_single_category_and_boundary_changes():
    orc.check_categorical_rows_and_chunks(5, 3 * T + 17, None, kind="single")
    orc.check_categorical_rows_and_chunks(5, 3 * T + 17, None, kind="edges")
    orc.check_categorical_rows_and_chunks(65, 3 * T + 17, None, kind="edges")


# ---- 6. dtypes and views ----------------------------------------------------------------------------------------------------------
def _outputs(m, x, family=None, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ResultWarning)
        pred, nats = m.pred_and_update_sequence(x, code_length=True, **kw)
    to = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t          # noqa: E731
    hn = [np.copy(v) for v in m.get_hn_params().values()]
    return [to(pred), to(nats)] + hn + [np.copy(v) for v in m.get_p_params().values()]


@pytest.mark.parametrize("family, dtypes", [(xs.BERNOULLI, (np.uint8, np.int32, np.int64)), (xs.POISSON, (np.uint8, np.int32, np.int64)),
                                            (xs.EXPONENTIAL, (np.float32, np.float64)), (xs.NORMAL, (np.float32, np.float64))])
def test_dtypes_and_views(family, dtypes):
    """Predictions, code lengths and p_* do not depend on where the sample lies.  hn_* of the float families are
    update_posterior's bits for the same array: its statistics pass cuts the sample at 16-byte boundaries, so its
    rounding, not this pass's, follows the alignment."""
    n = T + 5
    n_hn = len(orc.HN[family])
    for dtype in dtypes:
        x = orc.sample(family, n, seed=9, dtype=dtype)
        want = _outputs(orc.model(family), x)
        for off in range(4):
            view = torch.zeros(n + 3, dtype=torch.from_numpy(x).dtype, device="cuda")[off:off + n]
            view.copy_(torch.from_numpy(x))
            assert view.storage_offset() == off
            got = _outputs(orc.model(family), view)
            if family in (xs.EXPONENTIAL, xs.NORMAL):
                assert got[2:2 + n_hn] == orc.hn_of(orc.model(family).update_posterior(view), family)
                got[2:2 + n_hn] = want[2:2 + n_hn]
            assert all(same_bits(a, b) for a, b in zip(got, want)), (family, dtype, off)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64])
def test_categorical_dtypes_views_and_row_stride(dtype):
    n, degree = T + 5, 5
    x = orc.cat_sample(degree, n, seed=9, dtype=dtype)
    want = _outputs(orc.cat_model(degree), x, onehot=False)
    for off in range(4):
        view = torch.zeros(n + 3, dtype=torch.from_numpy(x).dtype, device="cuda")[off:off + n]
        view.copy_(torch.from_numpy(x))
        got = _outputs(orc.cat_model(degree), view, onehot=False)
        assert all(same_bits(a, b) for a, b in zip(got, want)), (dtype, off)
    hot = np.eye(degree, dtype=dtype)[x]
    want = _outputs(orc.cat_model(degree), hot)
    assert same_bits(want[1], _outputs(orc.cat_model(degree), x, onehot=False)[1])
    wide = torch.zeros((n, degree + 3), dtype=torch.from_numpy(hot).dtype).cuda()
    wide[:, :degree] = torch.from_numpy(hot).cuda()
    wide[:, degree:] = 7          # (never read)
    view = wide[:, :degree]
    assert view.stride(0) == degree + 3
    got = _outputs(orc.cat_model(degree), view)
    assert all(same_bits(a, b) for a, b in zip(got, want))


# ---- 7. refused samples on the device path ------------------------------------------------------------------------------------------
BAD_VALUE = {xs.BERNOULLI: 2, xs.POISSON: -1, xs.EXPONENTIAL: 0.0}


@pytest.mark.parametrize("family", sorted(BAD_VALUE))
def test_refused_sample_on_the_device_path(family):
    n = 3 * T + 17
    for at in (0, n - 1, T):
        x = torch.from_numpy(orc.sample(family, n, seed=2)).cuda()
        x[at] = BAD_VALUE[family]
        m, twin = orc.model(family, orc.FLOAT_START["exp"]), orc.model(family, orc.FLOAT_START["exp"])
        before = [np.copy(v) for v in list(m.get_hn_params().values()) + list(m.get_p_params().values())]
        with pytest.raises(DataFormatError) as want:
            twin.update_posterior(x)
        with pytest.raises(DataFormatError) as got:
            m.pred_and_update_sequence(x, code_length=True)
        assert str(got.value) == str(want.value)
        after = [np.copy(v) for v in list(m.get_hn_params().values()) + list(m.get_p_params().values())]
        assert all(same_bits(a, b) for a, b in zip(before, after)) and m._seq_engine is None
        # the entry point is safe on its own: the value is counted, adds nothing and gets a NaN code length
        eng = m._seq_pass()
        params, code, status = eng.run(family, x, orc.FLOAT_START["exp"])
        assert int(status.cpu()[0]) == 1 and bool(torch.isnan(code[at])) and int(torch.isnan(code).sum()) == 1
        good = x.clone()
        good[at] = 1
        clean, _, _ = eng.run(family, good, orc.FLOAT_START["exp"])
        for got, want_p in zip(params, clean):          # nothing before or at the bad position depends on it
            assert same_bits(got[:at + 1].cpu().numpy(), want_p[:at + 1].cpu().numpy())


def test_refused_categorical_sample_on_the_device_path():
    n, degree = 3 * T + 17, 5
    for at in (0, n - 1, T):
        for onehot in (False, True):
            x = orc.cat_sample(degree, n, seed=2)
            if onehot:
                xd = torch.from_numpy(np.eye(degree, dtype=np.int64)[x]).cuda()
                xd[at, (x[at] + 1) % degree] = 1          # a row with two ones
            else:
                xd = torch.from_numpy(x).cuda()
                xd[at] = degree
            m, twin = orc.cat_model(degree), orc.cat_model(degree)
            with pytest.raises(DataFormatError) as want:
                twin.update_posterior(xd, onehot=onehot)
            with pytest.raises(DataFormatError) as got:
                m.pred_and_update_sequence(xd, "squared", onehot, code_length=True)
            assert str(got.value) == str(want.value)
            assert same_bits(m.hn_alpha_vec, twin.hn_alpha_vec) and same_bits(m.p_theta_vec, twin.p_theta_vec) and m._seq_engine is None
            eng = m._seq_pass()
            xa = eng.adopt(xd, "i", degree) if onehot else eng.adopt(xd, "i")
            _, code, counts, status = eng.run_categorical(xa, onehot, m.hn_alpha_vec, "argmax", True, chunk_bytes=8 * xs.work_len(xs.CATEGORICAL, degree, 1000))
            assert int(status.cpu()[0]) == 1 and bool(torch.isnan(code[at])) and int(torch.isnan(code).sum()) == 1
            want_counts = np.bincount(np.delete(x, at), minlength=degree)
            assert np.array_equal(counts.cpu().numpy(), want_counts)          # the carry holds the good positions only


# ---- 8. determinism and end state -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [xs.BERNOULLI, xs.POISSON, xs.EXPONENTIAL, xs.NORMAL])
def test_determinism_and_end_state(family):
    n = 200003
    x = orc.sample(family, n, seed=8)
    first, second = _outputs(orc.model(family), x), _outputs(orc.model(family), x)
    assert all(same_bits(a, b) for a, b in zip(first, second))
    m, up = orc.model(family), orc.model(family).update_posterior(x)
    m.pred_and_update_sequence(x, None, code_length=True)
    assert orc.hn_of(m, family) == orc.hn_of(up, family)
    for k in ("_n", "_sum_log_factorial"):
        if hasattr(m, k):
            assert getattr(m, k) == getattr(up, k) and getattr(m, k) != 0


def test_categorical_determinism_and_end_state():
    n, degree = 200003, 16
    x = orc.cat_sample(degree, n, seed=8, dtype=np.uint8)
    xd = torch.from_numpy(x).cuda()
    first, second = _outputs(orc.cat_model(degree), xd, onehot=False), _outputs(orc.cat_model(degree), xd, onehot=False)
    assert all(same_bits(a, b) for a, b in zip(first, second))
    m, up = orc.cat_model(degree), orc.cat_model(degree).update_posterior(x, onehot=False)
    m.pred_and_update_sequence(xd, "0-1", False)
    assert same_bits(m.hn_alpha_vec, up.hn_alpha_vec)


def test_pickle_after_first_use_drops_the_engine():
    import pickle
    x = orc.sample(xs.POISSON, 1000, seed=1)
    m = orc.model(xs.POISSON)
    assert "_seq_engine" not in m.__dict__
    m.pred_and_update_sequence(x[:500])
    assert isinstance(m._seq_engine, xs.SequencePass)
    c = pickle.loads(pickle.dumps(m))
    assert "_seq_engine" not in c.__dict__ and c._seq_engine is None and c._engine is None
    assert orc.hn_of(c, xs.POISSON) == orc.hn_of(m, xs.POISSON) and c._sum_log_factorial == m._sum_log_factorial
    assert same_bits(c.pred_and_update_sequence(x[500:]), m.pred_and_update_sequence(x[500:]))


def test_tensor_in_gives_device_tensors_out():
    x = torch.from_numpy(orc.sample(xs.NORMAL, 1000, seed=1)).cuda()
    pred, nats = orc.model(xs.NORMAL).pred_and_update_sequence(x, code_length=True)
    assert pred.is_cuda and nats.is_cuda and pred.dtype == torch.float64
    c = orc.cat_model(4)
    rows = c.pred_and_update_sequence(torch.from_numpy(orc.cat_sample(4, 1000)).cuda(), "KL", False)
    assert rows.is_cuda and tuple(rows.shape) == (1000, 4) and same_bits(c.p_theta_vec, rows[-1].cpu().numpy())
