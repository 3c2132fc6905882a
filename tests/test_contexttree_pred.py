"""calc_pred_logpdf without a GPU: the NumPy restatement against the reference's fixtures and the exact recursion, the
ctpred C ABI's tables and argument checks, and the method's host logic on the CPU stand-ins."""
import ctypes
import itertools
import pickle
import re

import numpy as np
import pytest
import torch

import contexttree_oracle as orc
import contexttree_pred_oracle as porc
import contexttree_sparse_oracle as sorc
from bayesml_amd import _ctpred as _binding     # noqa: F401  (without the engine nothing below means anything)
from conftest import load_golden
from test_capi_symbols import header_functions, header_text

DENSE = [c["name"] for c in orc.CASES]
SPARSE = [c["name"] for c in sorc.CASES]
P = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _ctpred():
    from bayesml_amd import _ctpred
    return _ctpred


def _model(k=3, D=3, g=0.4, sparse=False):
    m = _ct().LearnModel(k, D, g, np.arange(1, k + 1) / 2.0, tables="sparse" if sparse else "dense")
    return porc.use_cpu(m, sparse)


def _trained(k=3, D=3, n=200, sparse=False, seed=1):
    x = orc.planted_sample(k, n, np.random.default_rng(seed))
    return _model(k, D, sparse=sparse).update_posterior(x), x


# ---- the restatement against the reference -------------------------------------------------------------------------------
def _final_lookup(name, sparse):
    case = (sorc if sparse else orc).case_by_name(name)
    k, D = case["k"], case["D"]
    fx = load_golden(f"contexttree_pred_{'sparse_' if sparse else ''}{name}.npz")
    if sparse:
        get = porc.sparse_lookup(sorc.lists_to_nodes(sorc.stage_lists(fx, "final"), k, D), k, D)
    else:
        old = load_golden(f"contexttree_{name}.npz")
        get = porc.dense_lookup({n: old[f"final_{n}"] for n in ("g", "beta", "exists", "leaf")}, k, D)
    return case, fx, get


@pytest.mark.parametrize("name,sparse", [(n, False) for n in DENSE] + [(n, True) for n in SPARSE])
def test_restatement_reproduces_the_reference(name, sparse):
    case, fx, get = _final_lookup(name, sparse)
    k, D, y = case["k"], case["D"], fx["y"].astype(np.int64)
    assert len(y) == 3 * (D + 2) + 40 and list(fx["lengths"][:5]) == [0, 1, D, D + 1, 0] and fx["lengths"].sum() == len(y)
    for ref, lengths in ((fx["p_one"], None), (fx["p_split"], fx["lengths"])):
        rows = porc.pred_rows(y, lengths, k, D, get, float(fx["hn_g"]), fx["hn_beta_vec"])
        assert np.all(np.abs(rows - ref) <= porc.p_rel_reference(k, D) * ref)
        assert np.mean(~porc.z_clear(ref, k, D)) <= 0.02
        clear = porc.z_clear(ref, k, D)
        assert np.array_equal(rows.argmax(1)[clear], ref.argmax(1)[clear])
    if name in ("k2_d10", "k4_d4"):
        assert not np.array_equal(fx["p_one"], fx["p_split"])    # (the cut changes contexts)


@pytest.mark.parametrize("name,sparse", [(n, False) for n in DENSE] + [(n, True) for n in SPARSE])
def test_restatement_reproduces_the_old_fixtures_pred(name, sparse):
    mod = sorc if sparse else orc
    case = mod.case_by_name(name)
    k, D, inp = case["k"], case["D"], mod.case_inputs(case)
    fx = load_golden(f"contexttree_{'sparse_' if sparse else ''}{name}.npz")
    stage = "after2" if len(inp["x2"]) else "after1"
    if sparse:
        get = porc.sparse_lookup(sorc.lists_to_nodes(sorc.stage_lists(fx, stage), k, D), k, D)
    else:
        get = porc.dense_lookup({n: fx[f"{stage}_{n}"] for n in ("g", "beta", "exists", "leaf")}, k, D)
    hn2 = case.get("hn2")
    hn_g, hb = (hn2[0], np.array(hn2[1])) if hn2 else (case["h0_g"], np.arange(1, k + 1) / 2.0)
    for j in range(3):
        row = porc.pred_rows(inp[f"ctx{j}"], None, k, D, get, hn_g, hb)[-1]
        assert np.all(np.abs(row - fx[f"pred{j}"]) <= porc.p_rel_reference(k, D) * fx[f"pred{j}"]), j


@pytest.mark.parametrize("name", ["k2_d3", "k3_d2", "k4_d4", "hn_changed"])
def test_exact_version_agrees_with_the_restatement(name):
    mp = orc._mp()
    case, fx, get = _final_lookup(name, False)
    k, D, y = case["k"], case["D"], fx["y"].astype(np.int64)
    rows = porc.pred_rows(y, fx["lengths"], k, D, get, float(fx["hn_g"]), fx["hn_beta_vec"])
    exact = porc.pred_rows_exact(y, fx["lengths"], k, D, get, float(fx["hn_g"]), fx["hn_beta_vec"])
    lnp = porc.outputs(rows, y, fx["lengths"])[0]
    for i in range(len(y)):
        for a in range(k):
            assert abs(mp.mpf(float(rows[i, a])) - exact[i][a]) <= porc.p_rel_exact(k, D) * exact[i][a]
        assert abs(mp.mpf(float(lnp[i])) - mp.log(exact[i][int(y[i])])) <= float(porc.lnp_abs_exact(k, D, lnp[i]))


# ---- header, library, ctypes table --------------------------------------------------------------------------------------
def test_header_library_and_table_agree():
    cp = _ctpred()
    lib = cp.load_library()
    declared = header_functions("ctpred.h", "ctpred")
    assert sorted(cp.SYMBOLS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    text = header_text("ctpred.h")
    assert lib.ctpred_abi_version() == 1 == int(re.search(r"#define CTPRED_ABI_VERSION (\d+)", text).group(1))
    assert re.search(rf"#define CTPRED_TILE {cp.TILE}\b", text) and re.search(rf"#define CTPRED_PIECE {cp.PIECE}\b", text)
    for other in ("ctree.h", "ctsp.h", "ctseq.h"):
        assert "ctpred_" not in header_text(other)
    for k in (1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 256):
        assert lib.ctpred_group_width(k) == cp.group_width(k) == min(64, 1 << int(np.ceil(np.log2(k))))
    assert lib.ctpred_group_width(0) == -1 and lib.ctpred_group_width(257) == -1


def test_plan_pieces_is_the_library_s():
    cp = _ctpred()
    lib = cp.load_library()
    for lengths in ([0], [1], [0, 0, 5, 0], [4096], [4097, 0, 4095, 1], [10 ** 6, 3, 0]):
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        S = len(lengths)
        got = (ctypes.c_int64 * (S + 1))()
        total = lib.ctpred_plan_pieces((ctypes.c_int64 * (S + 1))(*off), S, got)
        assert list(got) == list(cp.plan_pieces(off)) and total == got[S] == sum(-(-v // cp.PIECE) for v in lengths)
    assert lib.ctpred_plan_pieces(None, 1, None) == -1
    assert lib.ctpred_plan_pieces((ctypes.c_int64 * 2)(0, -1), 1, None) == -1
    assert lib.ctpred_plan_pieces((ctypes.c_int64 * 2)(1, 2), 1, None) == -1


OFF = (ctypes.c_int64 * 4)(0, 2, 6, 14)          # capacities 2, 4, 8 at D = 2


def _dense(lib, dtype=0, x=P, n=10, seq=None, S=0, k=2, D=2, tree=1, beta=P, g=P, exists=P, rowsum=P, hn_g=0.5, hb=P, lnp=P,
           arg=None, rows=None, status=P):
    return lib.ctpred_pass_dense(dtype, x, n, seq, S, k, D, tree, beta, g, exists, rowsum, hn_g, hb, lnp, arg, rows, status, None)


def _sparse(lib, dtype=0, x=P, n=10, seq=None, S=0, k=2, D=2, tree=1, off=OFF, key=P, beta=P, g=P, exists=P, rowsum=P,
            hn_g=0.5, hb=P, up=0, lnp=P, arg=None, rows=None, status=P):
    return lib.ctpred_pass_sparse(dtype, x, n, seq, S, k, D, tree, off, key, beta, g, exists, rowsum, hn_g, hb, up, lnp, arg,
                                  rows, status, None)


COMMON = [
    (dict(k=0), 1, "k and D"), (dict(D=0), 1, "k and D"), (dict(n=0), 1, "n must be"), (dict(n=2 ** 31), 2, "2^31"),
    (dict(dtype=3), 1, "dtype"), (dict(x=None), 1, "null"), (dict(beta=None), 1, "null"), (dict(g=None), 1, "null"),
    (dict(exists=None), 1, "null"), (dict(rowsum=None), 1, "null"), (dict(hb=None), 1, "null"), (dict(status=None), 1, "null"),
    (dict(lnp=None), 1, "no output"), (dict(hn_g=-0.1), 1, "hn_g"), (dict(hn_g=float("nan")), 1, "hn_g"),
    (dict(seq=P, S=0), 1, "go together"), (dict(seq=None, S=2), 1, "go together"), (dict(k=257), 2, "not supported"),
    (dict(x=ctypes.c_void_p(4097), dtype=1), 1, "aligned"), (dict(lnp=ctypes.c_void_p(4100)), 1, "misaligned"),
]


@pytest.mark.parametrize("kw,code,word", COMMON + [(dict(k=2, D=24), 2, "not supported"), (dict(k=256, D=3), 2, "not supported")])
def test_dense_pass_argument_errors_without_a_gpu(kw, code, word):
    lib = _ctpred().load_library()
    assert _dense(lib, **kw) == code
    assert word in lib.ctpred_last_error().decode()


@pytest.mark.parametrize("kw,code,word", COMMON + [
    (dict(k=2, D=64), 2, "not supported"), (dict(k=256, D=8), 2, "not supported"), (dict(off=None), 1, "null"),
    (dict(key=None), 1, "null"), (dict(off=(ctypes.c_int64 * 4)(1, 3, 7, 15)), 1, "off[0]"),
    (dict(off=(ctypes.c_int64 * 4)(0, 2, 5, 13)), 1, "power of two"), (dict(up=2), 1, "upwalk"),
])
def test_sparse_pass_argument_errors_without_a_gpu(kw, code, word):
    lib = _ctpred().load_library()
    assert _sparse(lib, **kw) == code
    assert word in lib.ctpred_last_error().decode()


def test_rowsum_and_totals_argument_errors_without_a_gpu():
    lib = _ctpred().load_library()
    err = lambda: lib.ctpred_last_error().decode()       # noqa: E731
    assert lib.ctpred_rowsum_dense(0, 2, 1, P, P, P, P, None) == 1 and "k and D" in err()
    assert lib.ctpred_rowsum_dense(256, 3, 1, P, P, P, P, None) == 2 and "not supported" in err()
    assert lib.ctpred_rowsum_dense(2, 2, 1, None, P, P, P, None) == 1 and "null" in err()
    assert lib.ctpred_rowsum_dense(2, 2, 1, P, None, P, P, None) == 1 and "null" in err()
    assert lib.ctpred_rowsum_dense(2, 2, 0, None, None, None, P, None) == 1 and "null" in err()
    assert lib.ctpred_rowsum_dense(2, 2, 1, P, P, P, ctypes.c_void_p(4100), None) == 1 and "misaligned" in err()
    assert lib.ctpred_rowsum_sparse(2, 64, 1, OFF, P, P, P, P, P, None) == 2 and "not supported" in err()
    assert lib.ctpred_rowsum_sparse(2, 2, 1, None, P, P, P, P, P, None) == 1 and "null" in err()
    assert lib.ctpred_rowsum_sparse(2, 2, 1, OFF, None, P, P, P, P, None) == 1 and "null" in err()
    assert lib.ctpred_rowsum_sparse(2, 2, 1, OFF, P, P, P, P, None, None) == 1 and "null" in err()
    assert lib.ctpred_totals(P, 10, P, P, 0, 1, P, P, None) == 1 and "S >= 1" in err()
    assert lib.ctpred_totals(P, 10, P, P, 2, 11, P, P, None) == 1 and "more pieces" in err()
    assert lib.ctpred_totals(P, 10, None, P, 2, 1, P, P, None) == 1 and "null" in err()
    assert lib.ctpred_totals(P, 10, P, None, 2, 1, P, P, None) == 1 and "null" in err()
    assert lib.ctpred_totals(P, 10, P, P, 2, 1, P, None, None) == 1 and "null" in err()
    assert lib.ctpred_totals(P, 10, P, P, 2, 1, ctypes.c_void_p(4100), P, None) == 1 and "misaligned" in err()


def test_check_raises_the_family_s_message():
    from bayesml_amd._engine import EngineError
    cp = _ctpred()
    with pytest.raises(EngineError, match="ctpred_pass_dense: GMMVB_EINVAL: ctpred_pass_dense: k and D must be >= 1"):
        cp._check(_dense(cp.load_library(), k=0), "ctpred_pass_dense")


# ---- the method's host logic on the CPU stand-ins -------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 4, 0, 0, 30, 2, 0]


@pytest.mark.parametrize("sparse", [False, True])
def test_return_shapes_and_order_for_every_flag_combination(sparse):
    m, _ = _trained(sparse=sparse)
    y = orc.planted_sample(3, 40, np.random.default_rng(9))
    base = m.calc_pred_logpdf(y, lengths=LENGTHS)
    assert isinstance(base, np.ndarray) and base.dtype == np.float64 and base.shape == (40,)
    for assign, dist, tot in itertools.product([False, True], repeat=3):
        got = m.calc_pred_logpdf(y, lengths=LENGTHS, assign=assign, return_dist=dist, totals=tot)
        if not (assign or dist or tot):
            assert isinstance(got, np.ndarray)
            got = (got,)
        assert isinstance(got, tuple) and len(got) == 1 + assign + dist + tot
        assert np.array_equal(got[0], base)
        rest = list(got[1:])
        if assign:
            z = rest.pop(0)
            assert isinstance(z, np.ndarray) and z.dtype == np.int64 and z.shape == (40,)
        if dist:
            d = rest.pop(0)
            assert d.dtype == np.float64 and d.shape == (40, 3) and np.allclose(d.sum(1), 1, atol=1e-14)
            assert np.array_equal(np.log(d[np.arange(40), y]), base)
            if assign:
                assert np.array_equal(z, d.argmax(1))
        if tot:
            t = rest.pop(0)
            assert t.dtype == np.float64 and t.shape == (len(LENGTHS),) and t[0] == 0.0 and t[-1] == 0.0
            at = np.concatenate([[0], np.cumsum(LENGTHS)])
            np.testing.assert_allclose(t, [base[a:b].sum() for a, b in zip(at[:-1], at[1:])], rtol=0, atol=1e-12)
        assert not rest
    assert m._pred_pass.launch_info == "cpu stand-in" and m._pred_pass.calls == 9


def test_numpy_in_numpy_out_tensor_in_tensor_out():
    m, _ = _trained()
    y = np.array([0, 1, 2, 2, 1, 0, 1, 1])
    a = m.calc_pred_logpdf(y, assign=True)
    b = m.calc_pred_logpdf(torch.from_numpy(y), assign=True)
    assert all(isinstance(v, np.ndarray) for v in a) and all(isinstance(v, torch.Tensor) for v in b)
    assert np.array_equal(a[0], b[0].numpy()) and np.array_equal(a[1], b[1].numpy())
    for dt in (np.uint8, np.int32, np.int64):
        assert np.array_equal(m.calc_pred_logpdf(y.astype(dt)), a[0])
    one = m.calc_pred_logpdf(2)
    assert isinstance(one, np.ndarray) and one.shape == (1,) and one[0] == m.calc_pred_logpdf(np.array([2]))[0]
    for lengths in ([3, 5], np.array([3, 5]), torch.tensor([3, 5]), (3, 5), np.array([3, 5], dtype=np.uint8)):
        assert np.array_equal(m.calc_pred_logpdf(y, lengths=lengths), m.calc_pred_logpdf(y, lengths=[3, 5]))


@pytest.mark.parametrize("sparse", [False, True])
def test_it_is_the_calc_pred_dist_loop(sparse):
    import copy
    m, x = _trained(sparse=sparse)
    y = np.concatenate([x[50:70], np.random.default_rng(4).integers(0, 3, 20)])
    lengths = [0, 7, 4, 0, 29]
    lnp, z, dist = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True)
    at = np.concatenate([[0], np.cumsum(lengths)])
    loop = copy.deepcopy(m)
    for a, b in zip(at[:-1], at[1:]):
        for i in range(a, b):
            want = loop.calc_pred_dist(y[a:i + 1]).p_theta_vec
            assert np.all(np.abs(dist[i] - want) <= porc.p_rel_reference(3, 3) * want)
            assert z[i] == loop.make_prediction(loss="0-1") or not porc.z_clear(want[None], 3, 3)[0]
            assert abs(lnp[i] - np.log(want[y[i]])) <= porc.lnp_abs_reference(3, 3, lnp[i])


@pytest.mark.parametrize("x,exc,text", [
    (np.array([0, -1, 1]), "DataFormatError", None), (np.array([0, 3, 1]), "DataFormatError", "x.max() must smaller than c_k:3"),
    (np.array([3, 0, 1]), "DataFormatError", "x.max() must smaller than c_k:3"),
    (np.array([0, 1, 255], dtype=np.uint8), "DataFormatError", "x.max() must smaller than c_k:3"),
    (np.array([0, 3, -1]), "DataFormatError", None), (np.array([0.0, 1.0]), "DataFormatError", None),
    ([0, 1], "DataFormatError", None), (np.zeros(0, dtype=int), "ValueError", None),
])
@pytest.mark.parametrize("sparse", [False, True])
def test_refusals_are_update_posterior_s_and_change_nothing(x, exc, text, sparse):
    from bayesml_amd import _check
    m, _ = _trained(sparse=sparse)
    ref, _ = _trained(sparse=sparse)
    before, p_before, blob = m._store.save(m._eng()), m.p_theta_vec.copy(), pickle.dumps(m)
    got = orc.outcome(lambda: m.calc_pred_logpdf(x, assign=True))
    assert got[0] == exc and got == orc.outcome(lambda: ref.update_posterior(x))
    if exc == "DataFormatError":
        assert got[1] == (text or "x" + _check.SAMPLE_MSG["nonneg_ints"])
    after = m._store.save(m._eng())
    assert all(np.array_equal(before[n], after[n]) for n in before)
    assert np.array_equal(p_before, m.p_theta_vec) and pickle.dumps(m) == blob


def test_totals_without_lengths_is_refused():
    from bayesml_amd._exceptions import ParameterFormatError
    m, _ = _trained()
    with pytest.raises(ParameterFormatError, match="lengths"):
        m.calc_pred_logpdf(np.array([0, 1]), totals=True)


@pytest.mark.parametrize("lengths", [[3, -1, 2], [3, 2], [2, 1], [1.0, 3.0], np.array([[4]]), np.array(4), "4", [None], [[1], [3]],
                                      np.array([2.5, 1.5])])
def test_a_bad_lengths_is_refused_before_the_device(lengths):
    from bayesml_amd._exceptions import DataFormatError
    m = _ct().LearnModel(3, 3)                    # no stand-in: an engine would need a GPU
    with pytest.raises(DataFormatError, match="lengths must be"):
        m.calc_pred_logpdf(np.array([0, 1, 2, 1]), lengths=lengths)
    assert m._engine is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal without a GPU")
def test_no_cpu_fallback():
    from bayesml_amd._engine import EngineUnavailableError
    for tables in ("dense", "sparse"):
        with pytest.raises(EngineUnavailableError):
            _ct().LearnModel(3, 3, tables=tables).calc_pred_logpdf(np.array([0, 1, 2]))


@pytest.mark.parametrize("sparse", [False, True])
def test_nothing_changes(sparse):
    m, x = _trained(sparse=sparse)
    before, blob = m._store.save(m._eng()), pickle.dumps(m)
    hn = (m.hn_g, m.hn_beta_vec.copy(), m.p_theta_vec.copy())
    y = np.random.default_rng(8).integers(0, 3, 60)          # (contexts the sample never held: calc_pred_dist would add nodes)
    m.calc_pred_logpdf(y, lengths=[20, 40], assign=True, return_dist=True, totals=True)
    after = m._store.save(m._eng())
    assert all(np.array_equal(before[n], after[n]) for n in before) and pickle.dumps(m) == blob
    assert hn[0] == m.hn_g and np.array_equal(hn[1], m.hn_beta_vec) and np.array_equal(hn[2], m.p_theta_vec)
    m2 = porc.use_cpu(pickle.loads(blob), sparse)
    assert "_pred_pass" not in m2.__dict__ and np.array_equal(m2.calc_pred_logpdf(y), m.calc_pred_logpdf(y))


@pytest.mark.parametrize("sparse", [False, True])
def test_a_model_without_a_tree(sparse):
    m = _model(sparse=sparse)
    y = np.array([2, 0, 1, 1, 2])
    lnp, z, dist = m.calc_pred_logpdf(y, assign=True, return_dist=True)
    want = m.hn_beta_vec / m.hn_beta_vec.sum()
    assert np.array_equal(dist, np.tile(want, (5, 1))) and np.array_equal(z, np.full(5, 2))
    assert np.array_equal(lnp, np.log(want[y])) and m.hn_root is None


def test_dense_and_sparse_stand_ins_agree():
    (a, x), (b, _) = _trained(sparse=False), _trained(sparse=True)
    y = np.concatenate([x[:30], np.random.default_rng(5).integers(0, 3, 30)])
    for u, v in zip(a.calc_pred_logpdf(y, lengths=LENGTHS + [20], assign=True, return_dist=True, totals=True),
                    b.calc_pred_logpdf(y, lengths=LENGTHS + [20], assign=True, return_dist=True, totals=True)):
        assert np.array_equal(u, v)
