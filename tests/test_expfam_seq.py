"""``pred_and_update_sequence`` of the five scalar conjugate models without a GPU: the Python layer through the NumPy
restatement of the pass (tests/expfam_seq_oracle.py), the restatement against the exact oracle and the per-value loop under
the bounds the GPU tests use, the reference's fixtures, and the argument checks of include/expseq.h."""
import ctypes
import pickle
import re
import warnings

import numpy as np
import pytest
import torch

import expfam_seq_oracle as orc
from conftest import load_golden
from expfam_seq_oracle import T, use_cpu
from test_capi_symbols import header_functions, header_text

from bayesml_amd import _expfam as xf
from bayesml_amd import _expseq as xs
from bayesml_amd import bernoulli, categorical, exponential, normal, poisson
from bayesml_amd._engine import EngineUnavailableError
from bayesml_amd._exceptions import CriteriaError, DataFormatError, ResultWarning

SCALAR = (xs.BERNOULLI, xs.POISSON, xs.EXPONENTIAL, xs.NORMAL)
CPU_LENGTHS = orc.EDGE_LENGTHS[:-1]


def _models():
    return [use_cpu(m) for m in (bernoulli.LearnModel(), categorical.LearnModel(3), poisson.LearnModel(),
                                 exponential.LearnModel(), normal.LearnModel())]


GOOD = [np.array([0, 1, 1, 0, 1]), np.array([2, 0, 1, 1, 2]), np.array([3, 0, 7, 2, 2]), np.array([0.5, 2.0, 1.25, 3.0, 0.1]),
        np.array([-1.0, 2.0, 0.25, 3.0, 1.5])]


def _call(m, x, loss="squared", **kw):
    if isinstance(m, categorical.LearnModel):
        kw.setdefault("onehot", False)
    return m.pred_and_update_sequence(x, loss, **kw)


def _state(m):
    s = {k: np.copy(v) for k, v in {**m.get_hn_params(), **m.get_p_params()}.items()}
    s.update({k: getattr(m, k) for k in ("_n", "_sum_log_factorial") if hasattr(m, k)})
    return s


def _same(a, b):
    return list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ---- the Python layer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tensor", [False, True])
@pytest.mark.parametrize("code_length", [False, True])
def test_return_types_and_shapes(tensor, code_length):
    kind = torch.Tensor if tensor else np.ndarray
    f64, i64 = (torch.float64, torch.int64) if tensor else (np.float64, np.int64)
    want = {bernoulli.LearnModel: {"squared": (f64, (5,)), "0-1": (i64, (5,)), "abs": (i64, (5,)), "KL": (f64, (5, 2))},
            categorical.LearnModel: {"squared": (f64, (5, 3)), "KL": (f64, (5, 3)), "0-1": (i64, (5,))},
            poisson.LearnModel: {"squared": (f64, (5,)), "0-1": (f64, (5,)), "abs": (np.float64, (5,)), "KL": None},
            exponential.LearnModel: {"squared": (f64, (5,)), "0-1": (f64, (5,)), "abs": (f64, (5,)), "KL": None},
            normal.LearnModel: {"squared": (f64, (5,)), "0-1": (f64, (5,)), "abs": (f64, (5,)), "KL": None}}
    for make, good in zip(_models(), GOOD):
        for loss, spec in want[type(make)].items():
            m = use_cpu(type(make)(*make.get_constants().values()))
            x = torch.from_numpy(good) if tensor else good
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ResultWarning)
                r = _call(m, x, loss, code_length=code_length)
            pred, nats = r if code_length else (r, None)
            if code_length:
                assert isinstance(nats, kind) and nats.dtype == f64 and tuple(nats.shape) == (5,)
            if spec is None:                       # a frozen SciPy distribution over the parameter arrays (host)
                assert pred.mean().shape == (5,)
            elif spec[0] is np.float64:            # SciPy's median (host)
                assert isinstance(pred, np.ndarray) and pred.shape == spec[1]
            else:
                assert isinstance(pred, kind) and pred.dtype == spec[0] and tuple(pred.shape) == spec[1], (type(m), loss)
    c = use_cpu(categorical.LearnModel(3))
    hot = np.eye(3, dtype=np.int64)[GOOD[1]]
    r = c.pred_and_update_sequence(torch.from_numpy(hot) if tensor else hot, "0-1")
    assert isinstance(r, kind) and r.dtype == i64 and tuple(r.shape) == (5, 3) and bool((r.sum(1) == 1).all())


def test_loss_none_leaves_p_and_other_losses_set_the_last_prediction():
    for m, good in zip(_models(), GOOD):
        m.update_posterior(good) if not isinstance(m, categorical.LearnModel) else m.update_posterior(good, onehot=False)
        m.calc_pred_dist()
        p0 = {k: np.copy(v) for k, v in m.get_p_params().items()}
        nats = _call(m, good, None, code_length=True)
        assert isinstance(nats, np.ndarray) and nats.shape == (5,) and _same(p0, m.get_p_params())
        eng = m._seq_pass()
        assert eng.calls[-1][3] in (False, None) and eng.calls[-1][4] is True          # no parameter arrays, no rows
        loop = type(m)(*m.get_constants().values())
        loop.set_hn_params(*m.get_hn_params().values())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ResultWarning)
            _call(m, good)
            for v in good:
                loop.pred_and_update(v.item(), **({"onehot": False} if isinstance(m, categorical.LearnModel) else {}))
        for k, v in loop.get_p_params().items():
            assert np.allclose(getattr(m, k), v, rtol=1e-14, atol=0), k


def test_criteria_errors():
    for m, good in zip(_models(), GOOD):
        before = _state(m)
        with pytest.raises(CriteriaError, match="loss=None returns the code lengths alone: pass code_length=True with it."):
            _call(m, good, None)
        for bad in ("KLD", 3, "abs" if isinstance(m, categorical.LearnModel) else "l1"):
            with pytest.raises(CriteriaError) as e:
                _call(m, good, bad)
            with pytest.raises(CriteriaError) as e2:
                m.make_prediction(bad)
            assert str(e.value) == str(e2.value)
        assert _same(before, _state(m)) and m._seq_pass().calls == []


REFUSED = [(0, np.array([0, -1, 1]), {}), (0, np.array([0, 2]), {}), (0, np.array([0.0, 1.0]), {}), (0, [0, 1], {}),
           (1, np.array([0, 3, 1]), {}), (1, np.array([0, -1]), {}), (1, np.array([[0, 1, 0], [1, 1, 0]]), {"onehot": True}),
           (1, np.array([[0, 1], [1, 0]]), {"onehot": True}), (1, np.zeros(0, dtype=np.int64), {}), (1, [1, 2], {}),
           (2, np.array([1, -2]), {}), (2, np.array([1.0, 2.0]), {}), (2, [1, 2], {}),
           (3, np.array([1.0, 0.0]), {}), (3, np.array([1.0, np.nan]), {}), (3, [1.0, 2.0], {}), (3, np.array(["a"]), {}),
           (4, [1.0, 2.0], {}), (4, np.array(["a"]), {})]


@pytest.mark.parametrize("which, bad, kw", REFUSED, ids=[f"{w}-{i}" for i, (w, _, _) in enumerate(REFUSED)])
def test_refused_sample_raises_what_update_posterior_raises_and_changes_nothing(which, bad, kw):
    m, twin = _models()[which], _models()[which]
    for model in (m, twin):
        model.update_posterior(GOOD[which], **({"onehot": False} if which == 1 else {}))
        model.calc_pred_dist()
    before = _state(m)
    up_kw = dict(kw) if which != 1 else {"onehot": kw.get("onehot", False)}
    with pytest.raises(Exception) as want:
        twin.update_posterior(bad, **up_kw)
    with pytest.raises(type(want.value)) as got:
        _call(m, bad, code_length=True, **kw)
    assert str(got.value) == str(want.value)
    assert _same(before, _state(m)) and m._seq_pass().calls == []


def test_empty_samples():
    for which, empty in ((0, np.zeros(0, dtype=np.int64)), (2, np.zeros(0, dtype=np.int64)), (3, np.zeros(0)), (4, np.zeros(0))):
        m = _models()[which]
        before = _state(m)
        pred, nats = _call(m, empty, code_length=True)
        assert pred.shape == (0,) and nats.shape == (0,) and pred.dtype == np.float64 and _same(before, _state(m))
        t = _call(m, torch.from_numpy(empty))
        assert isinstance(t, torch.Tensor) and t.shape == (0,)
    c = _models()[1]
    rows, nats = c.pred_and_update_sequence(np.zeros((0, 3), dtype=np.int64), code_length=True)
    assert rows.shape == (0, 3) and nats.shape == (0,)
    assert c.pred_and_update_sequence(np.zeros((0, 3), dtype=np.int64), "0-1").shape == (0, 3)
    with pytest.raises(ValueError):          # update_posterior's np.max of an empty index sample
        c.pred_and_update_sequence(np.zeros(0, dtype=np.int64), onehot=False)


def test_a_scalar_is_a_sample_of_one():
    for which, item in ((0, 1), (1, 2), (2, 4), (3, 0.5), (4, -1.25), (2, np.int64(3)), (4, np.float64(2.0))):
        m, loop = _models()[which], _models()[which]
        kw = {"onehot": False} if which == 1 else {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ResultWarning)
            pred, nats = _call(m, item, "0-1" if which == 1 else "abs", code_length=True)
            want = loop.pred_and_update(item, "0-1" if which == 1 else "abs", **kw)
        assert isinstance(pred, np.ndarray) and pred.shape[0] == 1 and nats.shape == (1,)
        assert np.array_equal(pred[0], want) and _same(_state(m), _state(loop))
    c, loop = _models()[1], _models()[1]
    row = np.array([0, 0, 1])
    assert np.array_equal(c.pred_and_update_sequence(row)[0], loop.pred_and_update(row)) and _same(_state(c), _state(loop))


def test_pickle_round_trip_before_and_after_first_use():
    for make, good in zip(_models(), GOOD):
        fresh = type(make)(*make.get_constants().values())
        assert "_seq_engine" not in fresh.__dict__ and "_expseq_pass_factory" not in fresh.__dict__
        assert fresh._seq_engine is None and fresh._expseq_pass_factory is None
        assert set(pickle.loads(pickle.dumps(fresh)).__dict__) == set(fresh.__dict__)
        m = type(make)(*make.get_constants().values())
        m._expfam_pass_factory = None
        m._seq_engine = object()                   # an engine never travels with the model
        c = pickle.loads(pickle.dumps(m))
        assert "_seq_engine" not in c.__dict__ and c._seq_engine is None and set(c.__dict__) == set(fresh.__dict__)
        # a model that has used the method (through the stand-in; tests/test_gpu_expfam_seq.py does it with the real engine)
        first = _call(make, good, None, code_length=True)
        make._seq_engine = object()
        used = pickle.loads(pickle.dumps(make))
        assert "_seq_engine" not in used.__dict__ and used._engine is None and _same(_state(used), _state(make))
        assert np.array_equal(_call(used, good, None, code_length=True), _call(make, good, None, code_length=True))
        assert first.shape == (5,)


def test_exponential_mean_is_nan_with_one_warning():
    m = use_cpu(exponential.LearnModel(h0_alpha=0.5))
    with pytest.warns(ResultWarning) as rec:
        pred = m.pred_and_update_sequence(GOOD[3])
    assert len(rec) == 1 and np.isnan(pred[0]) and np.all(np.isfinite(pred[1:]))


# ---- the restatement against the exact oracle and the loop: the bounds of the GPU tests, checked here first ----------------
@pytest.mark.parametrize("n", CPU_LENGTHS)
@pytest.mark.parametrize("family", [xs.BERNOULLI, xs.POISSON])
def test_integer_state_is_exact(family, n):
    orc.check_integer_state(family, n, use_cpu, with_loop=True)


@pytest.mark.parametrize("degree, n", [(1, 5), (2, 1), (3, 2), (5, T + 1), (3, 3 * T + 17)])
def test_categorical_integer_state_is_exact(degree, n):
    orc.check_categorical_integer_state(degree, n, use_cpu)


@pytest.mark.parametrize("n", orc.EDGE_LENGTHS)
def test_float_state_within_the_derived_bounds(n):
    for dtype in (np.float32, np.float64):
        orc.check_float_state(xs.EXPONENTIAL, n, dtype, None, use_cpu)
        for recipe in ("std", "tight", "offset"):
            orc.check_float_state(xs.NORMAL, n, dtype, recipe, use_cpu)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_state_against_the_loop(dtype):
    orc.check_against_loop(xs.EXPONENTIAL, dtype, None, use_cpu)
    for recipe in ("std", "tight", "offset"):
        orc.check_against_loop(xs.NORMAL, dtype, recipe, use_cpu)


def test_the_tight_recipe_needs_the_pivot():
    """Without the pivot the merge carries means of 1e6 for a spread of 1e-2 and the bound on beta is missed."""
    x = orc.sample(xs.NORMAL, 3 * T + 17, seed=1, recipe="tight")
    cnt, mean, m2 = orc.exclusive_prefix(orc.MergeOp(), (np.ones(x.shape[0]), x.copy(), np.zeros(x.shape[0])), x.shape[0])
    ex = orc.Exact(xs.NORMAL, x, orc.FLOAT_START["tight"])
    i = x.shape[0] - 1
    s1 = orc._frac(ex.s1[i], ex.e)
    m2_exact = orc._frac(ex.s2[i], 2 * ex.e) - s1 * s1 / i
    bound = orc.normal_bounds(x, orc.FLOAT_START["tight"], i, orc.longest_path(x.shape[0]), 0.0, 0.0)[1]
    assert abs(orc.Fraction(float(m2[i])) - m2_exact) / 2 > bound


def test_code_lengths_within_their_bounds():
    n = 3 * T + 17
    for family, start in ((xs.BERNOULLI, (0.5, 0.5)), (xs.POISSON, (1.0, 1.0)), (xs.EXPONENTIAL, (1.0, 1.0)),
                          (xs.NORMAL, (0.0, 1.0, 1.0, 1.0))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ResultWarning)
            print("family", family, "worst error / bound", orc.check_nats(family, orc.sample(family, n, seed=3), start, use_cpu))
    for family, start in orc.LONG_START.items():
        print("family", family, "long posterior", orc.check_nats(family, orc.sample(family, n, seed=4), start, use_cpu))
    print("categorical", orc.check_categorical_nats(5, n, use_cpu), orc.check_categorical_nats(300, n, use_cpu))


def test_categorical_rows_argmax_and_chunks():
    orc.check_categorical_rows_and_chunks(5, 3 * T + 17, use_cpu)
    orc.check_categorical_rows_and_chunks(64, 3 * T + 17, use_cpu, kind="edges")


@pytest.mark.parametrize("name", sorted(orc.FIXTURES))
def test_reference_fixture(name):
    orc.check_fixture(name, load_golden(f"expfam_seq_{name}.npz"), use_cpu)


@pytest.mark.parametrize("degree", [3, 300])
def test_reference_fixture_categorical(degree):
    orc.check_categorical_fixture(degree, load_golden(f"expfam_seq_categorical_d{degree}.npz"), use_cpu)


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------
def test_header_library_and_table_agree():
    lib = xs.load_library()
    declared = header_functions("expseq.h", "expseq")
    assert sorted(xs.SYMBOLS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    text = header_text("expseq.h")
    assert lib.expseq_abi_version() == 1 == int(re.search(r"#define EXPSEQ_ABI_VERSION (\d+)", text).group(1))
    assert re.search(rf"#define EXPSEQ_TILE {xs.TILE}\b", text) and re.search(rf"#define EXPSEQ_SCAN_THREADS {xs.SCAN_THREADS}\b", text)
    assert xs.TILE == xs.THREADS * xs.ITEMS
    body = re.sub(r"\s+", " ", text)
    for name, (_, args) in xs.SYMBOLS.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1).strip()
        assert (0 if proto == "void" else proto.count(",") + 1) == len(args), name
    assert "expseq_" not in header_text("expfam.h") and xf.load_library().expfam_abi_version() == 1


def test_work_len_against_its_restatement():
    lib = xs.load_library()
    for family in range(-1, 7):
        for degree in (0, 1, 5, xf.MAX_DEGREE, xf.MAX_DEGREE + 1):
            for m in (-1, 0, 1, T - 1, T, T + 1, 10 ** 8, 2 ** 40):
                assert lib.expseq_work_len(family, degree, m) == xs.work_len(family, degree, m), (family, degree, m)
    assert xs.work_len(xs.NORMAL, 0, T + 1) == 16 and xs.work_len(xs.CATEGORICAL, 5, T + 1) == 2 * 6 + T + 1
    for degree in (1, 5, 300, xf.MAX_DEGREE):
        for m in (1, 7, T - 1, T, T + 1, 5 * T, 5 * T + 3):
            budget = 8 * xs.work_len(xs.CATEGORICAL, degree, m)
            assert xs.chunk_len(degree, budget) == m and xs.chunk_len(degree, budget + 7) == m, (degree, m)
            assert 8 * xs.work_len(xs.CATEGORICAL, degree, xs.chunk_len(degree, budget + 8)) <= budget + 8
    assert xs.chunk_len(4096, 1) == 1 and 8 * xs.work_len(xs.CATEGORICAL, 4096, xs.chunk_len(4096)) <= 256 << 20


def test_argument_errors_without_a_gpu():
    """Every argument is checked before anything touches the device: the pointers below are never dereferenced."""
    lib = xs.load_library()
    p = ctypes.c_void_p(4096)
    EINVAL, EUNSUPPORTED = 1, 2
    two, four = (ctypes.c_double * 2)(1.0, 1.0), (ctypes.c_double * 4)(0.0, 1.0, 1.0, 1.0)
    calls = {"expseq_bernoulli": (xf.U8, two, 2), "expseq_poisson": (xf.I64, two, 3), "expseq_exponential": (xf.F32, two, 3),
             "expseq_normal": (xf.F64, four, 4)}
    for name, (good, start, n_out) in calls.items():
        fn = getattr(lib, name)
        outs = (p,) * n_out
        assert fn(good, p, 0, start, *outs, p, p, None) == EINVAL and b"n must be" in lib.expseq_last_error()
        assert fn(7, p, 10, start, *outs, p, p, None) == EINVAL and b"dtype" in lib.expseq_last_error()
        assert fn(xf.F64 if good <= xf.I64 else xf.I32, p, 10, start, *outs, p, p, None) == EINVAL
        assert fn(good, None, 10, start, *outs, p, p, None) == EINVAL and b"null" in lib.expseq_last_error()
        assert fn(good, p, 10, None, *outs, p, p, None) == EINVAL
        assert fn(good, p, 10, start, *outs, None, p, None) == EINVAL and fn(good, p, 10, start, *outs, p, None, None) == EINVAL
        assert fn(good, p, 10, start, *((ctypes.c_void_p(4100),) + outs[1:]), p, p, None) == EINVAL
        assert b"aligned" in lib.expseq_last_error()
        bad = type(start)(*start)
        bad[len(start) - 1] = 0.0
        assert fn(good, p, 10, bad, *outs, p, p, None) == EINVAL and b"start" in lib.expseq_last_error()
        bad[len(start) - 1] = float("nan")
        assert fn(good, p, 10, bad, *outs, p, p, None) == EINVAL
    assert lib.expseq_normal(xf.F64, ctypes.c_void_p(4100), 10, four, p, p, p, p, p, p, None) == EINVAL
    cat = lambda **k: lib.expseq_categorical(*[{**dict(dtype=xf.I32, x=p, m=10, degree=4, onehot=0, ld=4, alpha=p, s0=2.0, i0=0,      # noqa: E731
                                                       counts=p, nats=p, rows=p, argmax=p, status=p, work=p, stream=None), **k}[a]
                                               for a in ("dtype", "x", "m", "degree", "onehot", "ld", "alpha", "s0", "i0", "counts",
                                                         "nats", "rows", "argmax", "status", "work", "stream")])
    assert cat(degree=0) == EINVAL and b"degree" in lib.expseq_last_error()
    assert cat(degree=xf.MAX_DEGREE + 1) == EUNSUPPORTED
    assert cat(dtype=xf.F32) == EINVAL and cat(m=0) == EINVAL and cat(i0=-1) == EINVAL
    assert cat(onehot=1, ld=3) == EINVAL and b"ld" in lib.expseq_last_error()
    assert cat(x=None) == EINVAL and cat(alpha=None) == EINVAL and cat(counts=None) == EINVAL and cat(work=None) == EINVAL
    assert cat(s0=0.0) == EINVAL and cat(s0=float("inf")) == EINVAL and b"s0" in lib.expseq_last_error()
    assert cat(rows=ctypes.c_void_p(4100)) == EINVAL and b"aligned" in lib.expseq_last_error()


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        return                              # (an unmarked test does not touch the device)
    with pytest.raises(EngineUnavailableError):
        xs.SequencePass()
    for m, good in zip([bernoulli.LearnModel(), categorical.LearnModel(3), poisson.LearnModel(), exponential.LearnModel(),
                        normal.LearnModel()], GOOD):
        with pytest.raises(EngineUnavailableError):
            _call(m, good)
        from fake_expfam_engine import cpu_factory
        m._expfam_pass_factory = cpu_factory          # the statistics pass accepted: the sequence pass itself refuses
        with pytest.raises(EngineUnavailableError, match="sequence passes need an MI355X"):
            _call(m, good)
        assert _same(m.get_hn_params(), type(m)(*m.get_constants().values()).get_hn_params())
