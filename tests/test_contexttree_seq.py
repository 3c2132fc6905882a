"""pred_and_update_sequence without a GPU: the NumPy restatement against the reference's fixtures, the chunk planner, the
ctseq C ABI's tables and argument checks, and the method's host logic on the CPU stand-ins."""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import contexttree_oracle as orc
import contexttree_seq_oracle as seq
from conftest import load_golden
from test_capi_symbols import header_functions, header_text

NAMES = [c["name"] for c in orc.CASES]
P = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _ctseq():
    from bayesml_amd import _ctseq
    return _ctseq


def _model(k=3, D=3, g=0.5, **kw):
    return seq.use_cpu(_ct().LearnModel(k, D, g, np.arange(1, k + 1) / 2.0, **kw))


# ---- helper (a) against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference_trace(name):
    ct = _ct()
    case, fx = orc.case_by_name(name), load_golden(f"contexttree_{name}.npz")
    k, D, tr = case["k"], case["D"], orc.case_inputs(case)["trace_x"]
    t = orc.prior_tables(ct, case)
    rows, nats = seq.sequence(tr, k, D, t, case["h0_g"], np.arange(1, k + 1) / 2.0)
    ex = fx["trace0_exists"] != 0
    assert np.max(np.abs(rows - fx["trace0_p"])) <= orc.trace_p_atol(0.0, D)
    assert np.array_equal(t["exists"], fx["trace0_exists"]) and np.array_equal(t["leaf"][ex], fx["trace0_leaf"][ex])
    assert np.array_equal(t["beta"][ex], fx["trace0_beta"][ex])
    assert orc.trace_g_ok(t["g"], fx["trace0_g"], fx["trace0_exists"], tol=0)
    np.testing.assert_allclose(nats, -np.log(fx["trace0_p"][np.arange(len(tr)), tr]), rtol=0, atol=1e-13)


@pytest.mark.parametrize("m", [1, 2, 7, 64])
def test_restatement_in_chunks(m):
    k, D, n = 3, 3, 300
    x = orc.planted_sample(k, n, np.random.default_rng(5))
    prior = np.arange(1, k + 1) / 2.0
    a, b = orc.new_tables(k, D), orc.new_tables(k, D)
    ra, _ = seq.sequence(x, k, D, a, 0.4, prior)
    rb, _ = seq.sequence(x, k, D, b, 0.4, prior, m=m)
    assert np.max(np.abs(ra - rb)) <= 2 * orc.trace_p_atol(0.0, D, steps=n)
    assert np.array_equal(a["exists"], b["exists"]) and np.array_equal(a["beta"], b["beta"])
    assert np.array_equal(a["leaf"], b["leaf"]) and orc.trace_g_ok(b["g"], a["g"], a["exists"], tol=0, steps=n)


# ---- plan_chunks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_rows", [False, True])
@pytest.mark.parametrize("n,k,D", [(1, 2, 3), (4100, 2, 6), (10 ** 6, 2, 10), (10 ** 5, 256, 2), (3 * 10 ** 9, 4, 6)])
def test_plan_chunks(n, k, D, want_rows):
    cs = _ctseq()
    for budget in (None, 0, 1000, 1 << 20, 1 << 28, 1 << 40):
        m = cs.plan_chunks(n, k, D, want_rows, budget)
        assert 1 <= m <= min(n, 2 ** 31 - 1)
        limit = cs.DEFAULT_CHUNK_BYTES if budget is None else budget
        if m > 1:
            assert 8 * cs.work_slots(k, D, m, want_rows) <= limit
        if m < min(n, 2 ** 31 - 1):
            assert 8 * cs.work_slots(k, D, m + 1, want_rows) > limit
        cuts = list(range(0, n, m)) if n // m < 10 ** 5 else None
        if cuts is not None:
            assert sum(min(m, n - b) for b in cuts) == n and cuts[0] == 0 and all(b % m == 0 for b in cuts)
    assert cs.plan_chunks(n, k, D, want_rows, 8 * cs.work_slots(k, D, 7, want_rows)) == min(7, n)


def test_work_slots_is_the_library_s():
    cs = _ctseq()
    lib = cs.load_library()
    for k, D in ((1, 2), (2, 10), (4, 6), (256, 2), (3, 7)):
        for m in (1, 2, 255, 256, 257, 4097, 10 ** 6 + 3):
            for rows in (0, 1):
                assert lib.ctseq_work_len(k, D, m, rows) == cs.work_slots(k, D, m, bool(rows))
    assert lib.ctseq_work_len(2, 2, 0, 0) == -1 and lib.ctseq_work_len(2, 2, 2 ** 31, 0) == -1
    assert lib.ctseq_work_len(257, 1, 10, 0) == -1 and lib.ctseq_work_len(0, 1, 10, 0) == -1


# ---- header, library, ctypes table --------------------------------------------------------------------------------------
def test_header_library_and_table_agree():
    cs = _ctseq()
    lib = cs.load_library()
    declared = header_functions("ctseq.h", "ctseq")
    assert sorted(cs.SYMBOLS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    text = header_text("ctseq.h")
    assert lib.ctseq_abi_version() == 1 == int(re.search(r"#define CTSEQ_ABI_VERSION (\d+)", text).group(1))
    assert re.search(rf"#define CTSEQ_TILE {cs.TILE}\b", text) and re.search(rf"#define CTSEQ_ROW_BLOCK {cs.ROW_BLOCK}\b", text)
    assert "ctseq_" not in header_text("ctree.h") and "ctseq_" not in header_text("ctsp.h")
    from bayesml_amd import _ctree, _ctsp
    assert _ctree.load_library().ctree_abi_version() == 1 and _ctsp.load_library().ctsp_abi_version() == 1


def _pass(lib, k=2, D=2, n=10, begin=0, m=10, beta=P, g=P, exists=P, leaf=P, hn_g=0.5, hb=P, work=P, x=P, dtype=0):
    return lib.ctseq_pass(dtype, x, n, begin, m, k, D, beta, g, exists, leaf, hn_g, hb, None, None, P, work, None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(k=0), 1, "k and D"), (dict(D=0), 1, "k and D"), (dict(m=0), 1, "n and m"), (dict(begin=5, m=6), 1, "begin + m"),
    (dict(beta=None), 1, "null"), (dict(g=None), 1, "null"), (dict(exists=None), 1, "null"), (dict(leaf=None), 1, "null"),
    (dict(hb=None), 1, "null"), (dict(work=None), 1, "null"), (dict(x=None), 1, "null"), (dict(dtype=3), 1, "dtype"),
    (dict(hn_g=1.5), 1, "hn_g"), (dict(k=257), 2, "not supported"), (dict(k=2, D=24), 2, "not supported"),
    (dict(k=256, D=3), 2, "not supported"), (dict(x=ctypes.c_void_p(4097), dtype=1), 1, "aligned"),
])
def test_argument_errors_without_a_gpu(kw, code, word):
    lib = _ctseq().load_library()
    assert _pass(lib, **kw) == code
    assert word in lib.ctseq_last_error().decode()


def test_check_raises_the_family_s_message():
    from bayesml_amd._engine import EngineError
    cs = _ctseq()
    with pytest.raises(EngineError, match="ctseq_pass: GMMVB_EINVAL: ctseq_pass: k and D must be >= 1"):
        cs._check(_pass(cs.load_library(), k=0), "ctseq_pass")


# ---- the method's host logic on the CPU stand-ins -------------------------------------------------------------------------
def test_return_types_and_shapes():
    n, k = 40, 3
    x = orc.planted_sample(k, n, np.random.default_rng(1))
    p = _model().pred_and_update_sequence(x)
    assert isinstance(p, np.ndarray) and p.dtype == np.float64 and p.shape == (n, k)
    am = _model().pred_and_update_sequence(x, loss="0-1")
    assert isinstance(am, np.ndarray) and am.dtype == np.int64 and am.shape == (n,) and np.array_equal(am, p.argmax(1))
    p2, nats = _model().pred_and_update_sequence(x, code_length=True)
    assert np.array_equal(p, p2) and nats.dtype == np.float64 and nats.shape == (n,)
    np.testing.assert_allclose(nats, -np.log(p[np.arange(n), x]), rtol=0, atol=1e-14)
    am2, nats2 = _model().pred_and_update_sequence(x, loss="0-1", code_length=True)
    assert np.array_equal(am, am2) and np.array_equal(nats, nats2)
    only = _model().pred_and_update_sequence(x, loss=None, code_length=True)
    assert isinstance(only, np.ndarray) and np.array_equal(only, nats)
    pt, nt = _model().pred_and_update_sequence(torch.from_numpy(x), code_length=True)
    assert isinstance(pt, torch.Tensor) and isinstance(nt, torch.Tensor) and np.array_equal(pt.numpy(), p)
    one = _model().pred_and_update_sequence(2)
    assert one.shape == (1, k)


def test_it_is_the_loop():
    n, k, D = 120, 3, 3
    x = orc.planted_sample(k, n, np.random.default_rng(2))
    a, b = _model(k, D, 0.3), _model(k, D, 0.3)
    for m in (a, b):
        m.update_posterior(x[:50])
        m.set_hn_params(0.35)
    loop = np.stack([a.pred_and_update(x[:i + 1]).copy() for i in range(n)])
    got = b.pred_and_update_sequence(x, chunk_bytes=8 * _ctseq().work_slots(k, D, 7, False))
    assert b._seq_pass.passes == -(-n // 7)
    assert np.max(np.abs(loop - got)) <= 2 * orc.trace_p_atol(0.0, D, steps=n)
    ta, tb = a._eng().get_tables(), b._eng().get_tables()
    ex = ta["exists"] != 0
    assert np.array_equal(ta["exists"], tb["exists"]) and np.array_equal(ta["beta"][ex], tb["beta"][ex])
    assert np.array_equal(ta["leaf"][ex], tb["leaf"][ex]) and orc.trace_g_ok(tb["g"], ta["g"], ta["exists"], tol=0, steps=n)
    assert np.array_equal(b.p_theta_vec, got[-1])


def test_loss_values():
    from bayesml_amd._exceptions import CriteriaError
    x = np.array([0, 1, 2, 1])
    with pytest.raises(CriteriaError):
        _model().pred_and_update_sequence(x, loss=None)
    for bad in ("squared", 0, "kl"):
        with pytest.raises(CriteriaError) as info:
            _model().pred_and_update_sequence(x, loss=bad)
        assert str(getattr(info.value, "value", info.value)) == \
            "Unsupported loss function! This function supports \"0-1\" and \"KL\"."
    m = _model()
    before = m.p_theta_vec.copy()
    m.pred_and_update_sequence(x, loss=None, code_length=True)
    assert np.array_equal(m.p_theta_vec, before) and m.hn_root is not None


def test_sparse_tables_are_refused():
    m = _ct().LearnModel(3, 3, tables="sparse")
    with pytest.raises(NotImplementedError, match="tables"):
        m.pred_and_update_sequence(np.array([0, 1]))


@pytest.mark.parametrize("x,exc,text", [
    (np.array([0, -1, 1]), "DataFormatError", None), (np.array([0, 3, 1]), "DataFormatError", "x.max() must smaller than c_k:3"),
    (np.array([0, 3, -1]), "DataFormatError", None), (np.array([0.0, 1.0]), "DataFormatError", None),
    ([0, 1], "DataFormatError", None), (np.zeros(0, dtype=int), "ValueError", None),
])
def test_a_refused_sample_changes_nothing(x, exc, text):
    from bayesml_amd import _check
    m, ref = _model(), _model()
    m.pred_and_update_sequence(np.array([0, 1, 2, 2, 1, 0, 1]))
    before, p_before = m._eng().get_tables(), m.p_theta_vec.copy()
    assert orc.outcome(lambda: m.pred_and_update_sequence(x))[0] == exc
    assert orc.outcome(lambda: m.pred_and_update_sequence(x)) == orc.outcome(lambda: ref.update_posterior(x))
    if exc == "DataFormatError":
        assert orc.outcome(lambda: m.pred_and_update_sequence(x))[1] == (text or "x" + _check.SAMPLE_MSG["nonneg_ints"])
    after = m._eng().get_tables()
    for name in ("g", "beta", "exists", "leaf"):
        assert np.array_equal(before[name], after[name])
    assert np.array_equal(p_before, m.p_theta_vec)
    fresh = _model()
    orc.outcome(lambda: fresh.pred_and_update_sequence(x))
    assert fresh.hn_root is None


def test_pickle_round_trip():
    x = orc.planted_sample(3, 60, np.random.default_rng(3))
    m = _model()
    m.pred_and_update_sequence(x[:30])
    m2 = seq.use_cpu(pickle.loads(pickle.dumps(m)))
    assert "_seq_pass" not in m2.__dict__
    a, b = m.pred_and_update_sequence(x[30:]), m2.pred_and_update_sequence(x[30:])
    assert np.array_equal(a, b)
    ta, tb = m._eng().get_tables(), m2._eng().get_tables()
    ex = ta["exists"] != 0
    assert np.array_equal(ta["exists"], tb["exists"]) and np.array_equal(ta["g"][ex], tb["g"][ex])


@pytest.mark.parametrize("g0", [0.5, 1 - 2.0 ** -20, 2.0 ** -30, 0.0, 1.0])
def test_restatement_against_the_exact_recursion(g0):
    """Helper (a) inside helper (b)'s bounds: h_g within g_bound(g, B), rows within the path's sum plus 8 (D + 1) eps."""
    mp = orc._mp()
    k, D, n, eps = 3, 3, 150, np.finfo(float).eps
    prior = np.arange(1, k + 1) / 2.0
    x = orc.planted_sample(k, n, np.random.default_rng(6))
    t = orc.new_tables(k, D)
    exact = seq.sequence_exact(x, k, D, orc.new_tables(k, D), g0, prior)
    rows, _ = seq.sequence(x, k, D, t, g0, prior)
    assert np.array_equal(t["exists"], exact["exists"])
    for i in np.flatnonzero(exact["exists"]):
        if exact["logit"][i] is None:
            assert t["g"][i] == float(exact["g"][i])
        else:
            assert abs(mp.mpf(float(t["g"][i])) - exact["g"][i]) <= orc.g_bound(exact["g"][i], exact["B"][i])
    for i in range(n):
        for a in range(k):
            assert abs(mp.mpf(float(rows[i, a])) - exact["p"][i][a]) <= exact["p_bound"][i] + 8 * (D + 1) * eps
