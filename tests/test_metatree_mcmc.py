"""metatree's MTMCMC / REMTMCMC without a GPU: the host side of ``LearnModel`` (preconditions, the chain's lists and counts,
g_max, the exchanges, the stdout protocol, the merge and the installed forest) through the CPU stand-in with growth
(tests/fake_metatree_grow_engine.py) against the NumPy restatement fed with the same addressed tables
(tests/metatree_mcmc_oracle.py), and the argument checks and the symbol table of include/mtgrow.h."""
import contextlib
import ctypes
import io
import pickle
import re

import numpy as np
import pytest

import fake_metatree_engine as fk
import fake_metatree_grow_engine as fg
import metatree_mcmc_oracle as mc
import metatree_oracle as orc
from test_capi_symbols import header_functions, header_text

EPS = np.finfo(float).eps


@pytest.fixture()
def mt():
    from bayesml_amd import metatree
    fg.use_cpu(metatree.LearnModel)
    yield metatree
    metatree.LearnModel._mtree_pass_factory = None


def _sample(n=160, seed=0, C=2):
    rng = np.random.default_rng(seed)
    xc = np.round(rng.uniform(-1, 1, (n, 2)), 3)
    xk = rng.integers(0, C, (n, 1))
    y = (rng.random(n) < np.where(xc[:, 1] < 0.1, 0.1, 0.9)).astype(int)
    return xc, xk, y


def _fit(m, xc, xk, y, alg, **kw):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        m.fit(xc, xk, y, alg_type=alg, **kw)
    return out.getvalue()


def _cfg(m, threshold_type="1d_kmeans"):
    return mc.Config(m._family, m._degree, m.c_dim_continuous, m.c_dim_categorical, int(m.c_num_children_vec[0]),
                     m.c_max_depth, m._prior_vec(), m._default_post(), m.hn_g, m.h0_g, threshold_type)


def _same_forest(got, want):
    for k, v in want.flat.arrays().items():
        assert np.array_equal(getattr(got.flat, k), v), k
    for k in ("g", "post", "lml", "lcm", "prob"):
        assert np.array_equal(got.state[k], want.state[k], equal_nan=True), k


# ---- the restatement against the reference's fixtures -------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_stream_oracle_reproduces_the_reference(case):
    """Mode (a): consuming ``default_rng(seed)`` as the reference does, the restatement makes every decision of the stored
    chain (accept flags, exchange list, the final structures and thresholds exactly) and its floats within 4 x the recorded
    reference-vs-restatement deviation + 64 eps."""
    from conftest import load_golden
    fx = load_golden(f"metatree_mcmc_{case['name']}.npz")
    inp = mc.case_inputs(case)
    for k, v in inp.items():
        assert np.array_equal(fx[k], v), k
    assert float(fx["margin"]) >= 1e-9
    tr, trees, prob = mc.run_case(case, mc.Stream(int(fx["seed"])))
    assert min(tr["margins"]) == float(fx["margin"])
    shape = fx["accept"].shape
    assert np.array_equal(np.array(tr["accept"], dtype=bool).reshape(shape), fx["accept"])
    assert list(tr.get("exchange", [])) == list(fx["exchange"])
    st = mc.stack(mc.case_config(case), trees)
    assert np.array_equal(st["feat"], fx["list_feat"]) and np.array_equal(st["thr"], fx["list_thr"])
    tol = {k: 4 * float(fx["ref_vs_oracle_" + k]) + 64 * EPS for k in ("L", "tp", "g", "post", "prob", "g_max")}
    scale = np.abs(fx["l_new"]).max()
    assert np.abs(np.array(tr["l_new"]).reshape(shape) - fx["l_new"]).max() <= tol["L"] * scale
    for key in ("tp_new", "tp_last"):
        got, want = np.array(tr[key]).reshape(shape), fx[key]
        same = got == want                       # (-inf where a kept node's g_max is 0)
        assert np.all(same | (np.abs(got - want) <= tol["tp"] * np.abs(want).max(initial=1.0, where=np.isfinite(want))))
    assert np.allclose(st["g"], fx["list_g"], rtol=tol["g"], atol=0) and np.allclose(prob, fx["prob"], rtol=tol["prob"], atol=0)
    assert np.allclose(st["post"], fx["list_post"], rtol=tol["post"], atol=tol["post"] * np.abs(fx["list_post"]).max())
    if case["alg"] == "MTMCMC":
        assert np.allclose(tr["g_max"], fx["g_max"], rtol=tol["g_max"], atol=0)


# ---- the chains through the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold_type, C", [("1d_kmeans", 2), ("sample_midpoint", 2), ("sample_midpoint", 3)])
def test_mtmcmc_through_the_model(mt, threshold_type, C):
    """The model's chain equals the restatement's on the same tables: accept flags, g_max trace, the list, prob_vec; and
    the stdout protocol byte for byte."""
    xc, xk, y = _sample(C=C)
    kw = dict(burn_in=12, num_metatrees=25)
    m = mt.LearnModel(2, 1, c_max_depth=2, c_num_children_vec=C)
    text = _fit(m, xc, xk, y, "MTMCMC", threshold_type=threshold_type, seed=5, **kw)
    cfg = _cfg(m, threshold_type)
    tr, trees, prob = mc.mtmcmc(cfg, xc, xk, y, mc.Addressed(5, 1, cfg.cap), **kw)
    out = np.array(m._mcmc_trace["out"])
    assert np.array_equal(out[:, 0, 0].astype(bool), np.array(tr["accept"], dtype=bool))
    assert np.array_equal(out[:, 0, 1], tr["l_new"]) and np.array_equal(out[:, 0, 2], tr["tp_new"])
    assert np.array_equal(out[:, 0, 3], tr["tp_last"]) and m._mcmc_trace["g_max"] == tr["g_max"]
    assert 0 < sum(tr["accept"]) < len(tr["accept"]), "the case must accept and reject"
    _same_forest(m._hn_forest(), m._forest_from_tables(trees, prob))
    assert len(m.hn_metatree_list) == len(trees) and abs(m.hn_metatree_prob_vec.sum() - 1) < 1e-14
    want, proposed, accepted = "brun_in: 12\n", 1, 1
    for i, ok in enumerate(tr["accept"]):
        proposed, accepted = proposed + 1, accepted + bool(ok)
        want += f"\r{proposed}(accepted:{accepted})"
        if proposed == 12:
            want += "\nburn_in + num_metatrees: 37\n"
    assert text == want + "\n"


@pytest.mark.parametrize("chains", [1, 2, 8])
def test_remtmcmc_through_the_model(mt, chains):
    xc, xk, y = _sample(seed=3)
    kw = dict(burn_in=9, num_metatrees=14, num_chains=chains, num_interval=3, num_exchange=4)
    m = mt.LearnModel(2, 1, c_max_depth=2)
    text = _fit(m, xc, xk, y, "REMTMCMC", seed=8, **kw)
    cfg = _cfg(m)
    tr, trees, prob = mc.remtmcmc(cfg, xc, xk, y, mc.Addressed(8, chains, cfg.cap, 4), **kw)
    out = np.array(m._mcmc_trace["out"])
    assert np.array_equal(out[:, :, 0].astype(bool), np.array(tr["accept"], dtype=bool))
    assert np.array_equal(out[:, :, 1], np.array(tr["l_new"]))
    assert m._mcmc_trace["exchange"] == tr["exchange"]
    if chains > 1:
        assert any(j >= 0 for j in tr["exchange"]), "the case must exchange"
    if chains == 8:
        assert chains - 2 in tr["exchange"] and any(0 <= j < chains - 2 for j in tr["exchange"]), "both branches of the exchange"
    _same_forest(m._hn_forest(), m._forest_from_tables(trees, prob))
    assert text == ("brun_in: 9\n" + "".join(f"\r{i}" for i in range(9)) + "\nnum_metatrees: 14\n"
                    + "".join(f"\r{i}" for i in range(14)) + "\n")


def test_the_installed_forest_serves_every_later_call(mt):
    """predict, predict_proba, estimate_params, feature importances, pickling and a later 'given_MT' update after a fit."""
    xc, xk, y = _sample(n=300)
    m = mt.LearnModel(2, 1, c_max_depth=2)
    _fit(m, xc, xk, y, "MTMCMC", burn_in=15, num_metatrees=30, seed=1)
    best = m.hn_metatree_list[int(np.argmax(m.hn_metatree_prob_vec))]
    assert not best.leaf and best.sub_model.hn_alpha + best.sub_model.hn_beta == 1.0 + len(y)
    acc = (m.predict(xc, xk) == y).mean()
    assert acc > max(y.mean(), 1 - y.mean()) + 0.1
    assert np.allclose(m.predict_proba(xc, xk).sum(1), 1.0)
    assert not m.estimate_params(visualize=False).leaf
    assert m.calc_feature_importances().argmax() == 1, "the planted feature carries the gain"
    m2 = pickle.loads(pickle.dumps(m))
    fg.use_cpu(m2)
    assert np.array_equal(m2.predict(xc, xk), m.predict(xc, xk))
    before = m._hn_forest().copy()
    x2, k2, y2 = _sample(n=60, seed=9)
    m.update_posterior(x2, k2, y2, alg_type="given_MT")
    want, _ = orc.batch_update(before.flat.arrays(), before.state, orc.BERNOULLI, 0, m._prior_vec(), 2, x2, k2, y2)
    for k in ("g", "post", "prob"):
        assert np.array_equal(m._hn_forest().state[k], want[k]), k


def test_one_feature_returns_the_initial_tree(mt):
    rng = np.random.default_rng(0)
    xc = rng.uniform(-1, 1, (80, 1))
    y = (xc[:, 0] > 0).astype(int)
    for alg, kw in (("MTMCMC", {}), ("REMTMCMC", dict(num_chains=3))):
        m = mt.LearnModel(1, 0, c_max_depth=2)
        text = _fit(m, xc, None, y, alg, seed=0, **kw)
        assert text == "" and len(m.hn_metatree_list) == 1 and np.array_equal(m.hn_metatree_prob_vec, [1.0])
        assert m.hn_metatree_list[0].k == 0


def test_a_seed_repeats_and_none_does_not(mt):
    xc, xk, y = _sample()
    runs = []
    for seed in (4, 4, None, None):
        m = mt.LearnModel(2, 1, c_max_depth=2)
        _fit(m, xc, xk, y, "MTMCMC", burn_in=8, num_metatrees=10, seed=seed)
        runs.append(np.array(m._mcmc_trace["out"]))
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[2], runs[3])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
REFUSED = [
    (dict(c_num_children_vec=np.array([2, 3, 2])), "MTMCMC", {},
     "MTMCMC is supported only when all the elements of self.c_num_children_vec are the same. self.c_num_children_vec = [2 3 2]."),
    (dict(c_num_assignment_vec=np.array([1, -1, -1])), "REMTMCMC", {},
     "MTMCMC is supported only when all the elements of self.c_num_assignment_vec are not positive. "
     "self.c_num_assignment_vec = [ 1 -1 -1]."),
    (dict(h0_k_weight_vec=np.array([1.0, 2.0, 1.0])), "MTMCMC", {},
     "MTMCMC is supported only when all the elements of self.h0_k_weight_vec are the same. self.h0_k_weight_vec = [1. 2. 1.]."),
    ({}, "MTMCMC", dict(threshold_type="even"), 'threshold_type must be "1d_kmeans" or "sample_midpoint".'),
    ({}, "REMTMCMC", dict(threshold_type="even"), 'threshold_type must be "1d_kmeans" or "sample_midpoint".'),
    ({}, "REMTMCMC", dict(beta_vec=np.array([0.5, 1.5]), num_chains=2),
     "All the elements of beta_vec must be in [0,1] beta_vec = [0.5 1.5]."),
    ({}, "REMTMCMC", dict(num_chains=0), "num_chains"),
    ({}, "REMTMCMC", dict(num_interval=0), "num_interval"),
    ({}, "REMTMCMC", dict(num_exchange=-1), "num_exchange"),
]


@pytest.mark.parametrize("consts, alg, kw, text", REFUSED, ids=[f"{r[1]}-{i}" for i, r in enumerate(REFUSED)])
def test_preconditions_and_an_untouched_state(mt, consts, alg, kw, text):
    """Every precondition's exception type and text; a refused call builds no engine and changes nothing."""
    from bayesml_amd._exceptions import ParameterFormatError
    xc, xk, y = _sample()
    m = mt.LearnModel(2, 1, c_max_depth=2, **consts)
    _fit(m, xc, xk, y, "MTRF", n_estimators=4, random_state=0) if not consts else None
    before = pickle.dumps((m.get_hn_params()["hn_metatree_prob_vec"], [t.k for t in m.hn_metatree_list]))
    built = []
    real = fg.CpuGrower.__init__
    fg.CpuGrower.__init__ = lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1]
    try:
        with pytest.raises(ParameterFormatError) as e:
            m.update_posterior(xc, xk, y, alg_type=alg, **kw)
    finally:
        fg.CpuGrower.__init__ = real
    # (the exception prints its message's repr, as the reference's does)
    assert (str(e.value) == repr(text)) if len(text) > 20 else (text in str(e.value))
    assert not built
    assert pickle.dumps((m.get_hn_params()["hn_metatree_prob_vec"], [t.k for t in m.hn_metatree_list])) == before


def test_capacity_limit_names_itself(mt):
    from bayesml_amd._engine import EngineLimitError
    xc, xk, y = _sample()
    m = mt.LearnModel(2, 1, c_max_depth=12)
    with pytest.raises(EngineLimitError, match="bayesml itself has no such limit"):
        m.update_posterior(xc, xk, y, alg_type="MTMCMC")
    m = mt.LearnModel(2, 1, c_max_depth=2)
    with pytest.raises(EngineLimitError, match="bayesml itself has no such limit"):
        m.update_posterior(xc, xk, y, alg_type="REMTMCMC", num_chains=1025)


def test_a_bad_categorical_value_is_refused_first(mt):
    from bayesml_amd._exceptions import DataFormatError
    xc, xk, y = _sample()
    xk = xk.copy()
    xk[3, 0] = 2
    m = mt.LearnModel(2, 1, c_max_depth=2)
    with pytest.raises(DataFormatError):
        m.update_posterior(xc, xk, y, alg_type="MTMCMC", burn_in=3, num_metatrees=3)
    assert m.hn_metatree_list == []


def test_a_factory_without_growth_and_no_gpu():
    """The plain stand-in has no grower: NotImplementedError names the alg_type.  Without a seam and without a GPU the call is
    EngineUnavailableError, like every other product path."""
    import torch
    from bayesml_amd import metatree
    from bayesml_amd._engine import EngineUnavailableError
    xc, xk, y = _sample()
    fk.use_cpu(metatree.LearnModel)
    try:
        with pytest.raises(NotImplementedError, match="REMTMCMC"):
            metatree.LearnModel(2, 1).update_posterior(xc, xk, y, alg_type="REMTMCMC")
    finally:
        metatree.LearnModel._mtree_pass_factory = None
    if not torch.cuda.is_available():
        with pytest.raises(EngineUnavailableError):
            metatree.LearnModel(2, 1).update_posterior(xc, xk, y, alg_type="MTMCMC")


# ---- the addressed tables ---------------------------------------------------------------------------------------------------
def test_draw_tables_are_the_documented_numpy_expressions():
    from bayesml_amd import _mtgrow
    want = np.random.Generator(np.random.Philox(key=9, counter=[0, 0, 4, 0])).random((3, 7, 2))
    assert np.array_equal(_mtgrow.node_table(9, 4, 3, 7), want) and np.array_equal(mc.node_table(9, 4, 3, 7), want)
    want = np.random.Generator(np.random.Philox(key=9, counter=[0, 0, 4, 1])).random(3 + 8)
    assert np.array_equal(_mtgrow.aux_table(9, 4, 3, 4), want) and np.array_equal(mc.aux_table(9, 4, 3, 4), want)
    # consecutive steps share no value (tables at consecutive FIRST counter words would share all but four)
    a, b = _mtgrow.node_table(9, 4, 3, 7).ravel(), _mtgrow.node_table(9, 5, 3, 7).ravel()
    assert not np.isin(a, b).any() and not np.isin(a, _mtgrow.aux_table(9, 4, 3, 4)).any()


# ---- include/mtgrow.h -----------------------------------------------------------------------------------------------------
def test_library_exports_every_symbol_of_mtgrow_h():
    """Header <-> .so <-> ctypes table, the ABI version in all three places, and mtree.h left at ABI 2."""
    from bayesml_amd import _mtgrow, _mtree
    lib = _mtgrow.load_library()
    declared = header_functions("mtgrow.h", "mtgrow")
    assert sorted(_mtgrow.SYMBOLS) == declared, "ctypes table and header disagree"
    for name in declared:
        assert getattr(lib, name) is not None
    text = header_text("mtgrow.h")
    assert lib.mtgrow_abi_version() == 1 == int(re.search(r"#define MTGROW_ABI_VERSION (\d+)", text).group(1))
    assert _mtgrow.KMEANS_BLOCK == int(re.search(r"#define MTGROW_KMEANS_BLOCK (\d+)", text).group(1))
    assert _mtree.load_library().mtree_abi_version() == 2 and "mtgrow_" not in header_text("mtree.h")
    fields = re.search(r"typedef struct mtgrow_state \{(.*?)\} mtgrow_state;", text, flags=re.S).group(1)
    names = re.findall(r"\b(\w+)\s*(?:,|;)", fields)
    assert names == [f[0] for f in _mtgrow.StateStruct._fields_], "struct mtgrow_state and its ctypes mirror disagree"


def test_capacity():
    from bayesml_amd import _mtgrow
    lib = _mtgrow.load_library()
    for C, d in ((2, 1), (2, 4), (3, 3), (4, 5), (2, 11), (16, 2)):
        assert lib.mtgrow_capacity(C, d) == _mtgrow.capacity(C, d) == mc.capacity(C, d)
    assert lib.mtgrow_capacity(2, 12) == -1 and lib.mtgrow_capacity(1, 2) == -1 and lib.mtgrow_capacity(2, 0) == -1


def test_argument_errors_without_a_gpu():
    """Every refusal is decided on the arguments alone (the pointers are never dereferenced)."""
    from bayesml_amd import _mtgrow
    from bayesml_amd._engine import EngineError
    lib = _mtgrow.load_library()
    P = 4096

    def state(**over):
        vals = dict(n_chains=2, cap=7, n_children=2, dim_cont=2, dim_cat=1, max_depth=2, n_post=2, threshold=_mtgrow.KMEANS,
                    n=100, xc_dtype=4, xk_dtype=0)
        vals.update({name: P for name, _ in _mtgrow.StateStruct._fields_ if name.endswith("_dev")})
        vals.update(over)
        return _mtgrow.StateStruct(**vals)

    def err(rc):
        assert rc != 0
        return rc, lib.mtgrow_last_error().decode()

    for over, code, text in ((dict(n_chains=0), 1, "n_chains"), (dict(n=0), 1, "n_chains, n and n_post"),
                             (dict(n=2 ** 31), 2, "2^31 - 1 rows"), (dict(n_chains=1025), 2, "1024 chains"),
                             (dict(max_depth=12, cap=8191), 2, "more than 4096 nodes"), (dict(cap=8), 1, "mtgrow_capacity"),
                             (dict(threshold=2), 1, "threshold"), (dict(xc_dtype=0), 1, "xc_dtype"), (dict(xk_dtype=4), 1, "xk_dtype"),
                             (dict(xc_dev=None), 1, "null sample pointer"), (dict(order_dev=None), 1, "null sample pointer"),
                             (dict(feat_dev=None), 1, "null table"), (dict(lo_dev=P + 4), 1, "misaligned"),
                             (dict(node_dev=P + 2), 1, "misaligned")):
        rc, msg = err(lib.mtgrow_level(ctypes.byref(state(**over)), 0, 0, 0.5, None))
        assert rc == code and text in msg, (over, msg)
    ok = state()
    assert err(lib.mtgrow_level(ctypes.byref(ok), 2, 0, 0.5, None)) == (1, "mtgrow_level: level must be 0 .. max_depth - 1")
    assert err(lib.mtgrow_level(ctypes.byref(ok), 0, 0, 1.5, None))[1] == "mtgrow_level: g_max must lie in [0, 1]"
    assert err(lib.mtgrow_level(None, 0, 0, 0.5, None))[1] == "mtgrow_level: null state"
    assert err(lib.mtgrow_begin(ctypes.byref(ok), 0.5, 0.5, None, None))[1] == "mtgrow_begin: null or misaligned sub_hn_dev"
    assert err(lib.mtgrow_begin(ctypes.byref(ok), 1.5, 0.5, P, None))[1] == "mtgrow_begin: g_root and g_below must lie in [0, 1]"
    args = [P] * 13
    assert err(lib.mtgrow_accept(ctypes.byref(ok), 0, 0.5, *args[:4], None, *args[5:], None))[1] == "mtgrow_accept: null pointer"
    assert err(lib.mtgrow_accept(ctypes.byref(ok), 0, 0.5, P + 4, *args[1:], None))[1] == "mtgrow_accept: misaligned pointer"
    assert err(lib.mtgrow_accept(ctypes.byref(ok), 0, -0.1, *args, None))[1] == "mtgrow_accept: g_max must lie in [0, 1]"
    with pytest.raises(EngineError, match="mtgrow_level: GMMVB_EINVAL: mtgrow_level: null state"):
        _mtgrow._check(lib.mtgrow_level(None, 0, 0, 0.5, None), "mtgrow_level")
