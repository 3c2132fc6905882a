"""``metatree`` with SubModel=linearregression without a GPU: the constructor rule, the host plumbing of the model over the
NumPy stand-in engine (tests/fake_metatree_lr_engine.py), the oracle (tests/metatree_lr_oracle.py) held to the reference's
fixtures (tests/golden/metatree_lr_*.npz), the argument checks of the new entry points of include/mtree.h, and that the edge
cases of tests/metatree_lr_cases.py reach what they name."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

import fake_metatree_lr_engine as fk
import metatree_lr_cases as lc
import metatree_lr_oracle as lro
import metatree_oracle as orc
from conftest import GOLDEN, load_golden

EPS = np.finfo(float).eps
CASE = {c["name"]: c for c in lro.CASES}


@pytest.fixture
def mt():
    from bayesml_amd import metatree
    fk.use_cpu(metatree.LearnModel)
    yield metatree
    metatree.LearnModel._mtree_pass_factory = None


@pytest.fixture
def lr():
    from bayesml_amd import linearregression
    return linearregression


# ---- the constructor rule -----------------------------------------------------------------------------------------------------
def test_constructor_rule(mt, lr):
    from bayesml_amd._engine import EngineLimitError
    for Model in (mt.LearnModel, mt.GenModel):
        with pytest.raises(EngineLimitError, match="linearregression.*c_degree"):
            Model(2, 0, SubModel=lr)                                          # no c_degree
        with pytest.raises(EngineLimitError, match="linearregression.*c_degree = 3 and c_dim_continuous = 2"):
            Model(2, 1, SubModel=lr, sub_constants={"c_degree": 3})
        with pytest.raises(EngineLimitError, match="linearregression.*c_dim_continuous = 0"):
            Model(0, 2, SubModel=lr, sub_constants={"c_degree": 1})
        with pytest.raises(EngineLimitError, match="linearregression.*bayesml itself has no such limit"):
            Model(16, 0, SubModel=lr, sub_constants={"c_degree": 16})
        for D in (1, 2, 15):
            m = Model(D, 1, SubModel=lr, sub_constants={"c_degree": D})
            assert m.get_constants()["sub_constants"] == {"c_degree": D}
    with pytest.raises(EngineLimitError) as e:
        mt.LearnModel(2, 0, SubModel=lr)
    assert "pass sub_constants={'c_degree': c_dim_continuous}" in str(e.value)


def test_limits_are_the_header_s():
    from bayesml_amd import _mtree
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mtree.h")).read()
    assert f"#define MTREE_LR_MAX_DEGREE {_mtree.LR_MAX_DEGREE}\n" in text and f"#define MTREE_LR_BLOCK {_mtree.LR_BLOCK}\n" in text
    assert "MTREE_LINREG = 5" in text and _mtree.LINREG == lro.LINREG == 5
    assert _mtree.stat_cols(_mtree.LINREG, 3) == (1, 6 + 3 + 1, 3 + 6 + 3) and lro.post_len(3) == 12
    assert "#define MTREE_ABI_VERSION 2\n" in text


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------
def test_new_entry_points_check_their_arguments():
    from bayesml_amd import _mtree
    lib = _mtree.load_library()
    ni, nr, npost = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for D in (1, 3, 15):
        assert lib.mtree_stat_cols(_mtree.LINREG, D, ni, nr, npost) == 0
        assert (ni.value, nr.value, npost.value) == _mtree.stat_cols(_mtree.LINREG, D)
    assert lib.mtree_stat_cols(_mtree.LINREG, 0, ni, nr, npost) == 1
    assert lib.mtree_stat_cols(_mtree.LINREG, 16, ni, nr, npost) == 2 and b"linear-regression degree above 15" in lib.mtree_last_error()
    assert lib.mtree_stat_cols(6, 3, ni, nr, npost) == 1
    assert lib.mtree_values_len(10, _mtree.LINREG, 3) == 10 * (3 + 6 + 2)
    assert lib.mtree_values_len(10, _mtree.NORMAL, 0) == 20 and lib.mtree_values_len(10, _mtree.CATEGORICAL, 5) == 50
    assert lib.mtree_values_len(0, _mtree.NORMAL, 0) == -1 and lib.mtree_values_len(10, _mtree.LINREG, 16) == -1
    B, nodes, n, S, D = 2, 10, 3 * _mtree.LR_BLOCK + 1, 4, 3
    nblk = 4
    want = (S * nodes + 1) // 2 + (nodes + 1) // 2 + (B + 1) // 2 + (B * n + 1) // 2 + B * nblk + B * nblk * 2 * 10
    assert lib.mtree_reduce_x_work_len(nodes, B, D, n, S) == want
    for bad in ((0, B, D, n, S), (nodes, 0, D, n, S), (nodes, B, 16, n, S), (nodes, B, D, 0, S), (nodes, B, D, 2 ** 31, S),
                (nodes, B, D, n, 65)):
        assert lib.mtree_reduce_x_work_len(*bad) == -1
    arr = (ctypes.c_int32 * 4)()
    p = ctypes.cast(arr, ctypes.c_void_p).value          # never dereferenced: every call below is refused on its arguments
    ok = _mtree.ForestStruct(1, 3, 3, 3, 2, 1, 3, 0, p, p, p, p, p, p, p)

    def reduce_x(family=_mtree.LINREG, degree=3, stop=p, dtype=_mtree.F64, x=p, stride=3, y=p, n=8, slabs=1, si=p, sr=p,
                 work=p):
        return lib.mtree_reduce_x(ctypes.byref(ok), family, degree, stop, dtype, x, stride, y, n, slabs, si, sr, work, None)
    for kw, text in ((dict(family=_mtree.NORMAL), b"only linear regression"), (dict(degree=16), b"degree above 15"),
                     (dict(degree=0), b"degree < 1"), (dict(n=0), b"n must be"), (dict(n=2 ** 31), b"n must be"),
                     (dict(slabs=65), b"n_slabs"), (dict(dtype=_mtree.I32), b"x_dtype"), (dict(stride=2), b"x_stride"),
                     (dict(x=None), b"null pointer"), (dict(work=None), b"null pointer"), (dict(y=p + 4), b"misaligned")):
        rc = reduce_x(**kw)
        assert rc == (2 if kw == dict(degree=16) else 1) and text in lib.mtree_last_error(), (kw, lib.mtree_last_error())
    assert lib.mtree_reduce(ctypes.byref(ok), _mtree.LINREG, 3, p, p, 8, 1, p, p, p, None) == 1
    assert b"use mtree_reduce_x" in lib.mtree_last_error()
    for mode in (_mtree.PRED_PROBA, _mtree.PRED_CLASS):
        assert lib.mtree_predict(ctypes.byref(ok), _mtree.LINREG, 3, mode, _mtree.F64, p, 0, None, 8, p, p, p, p, p, None) == 1
        assert b"no such read-out" in lib.mtree_last_error()
    assert lib.mtree_predict(ctypes.byref(ok), _mtree.LINREG, 2, _mtree.PRED_MEAN, _mtree.F64, p, 0, None, 8, p, p, p, p, p,
                             None) == 1 and b"must equal dim_cont" in lib.mtree_last_error()


def test_engine_limit_is_raised_before_the_device():
    from bayesml_amd import _mtree
    from bayesml_amd._engine import EngineLimitError
    flat = _mtree.FlatForest(**lc.forest([lc.STUMP]))
    with pytest.raises(EngineLimitError, match="linearregression up to c_degree = 15"):
        _mtree.MtreePass(flat, _mtree.LINREG, 16, 16, 0, [], lro.default_h0(16))
    _mtree.check_lr_degree(15)


# ---- the oracle against the reference's fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASE))
def test_fixture_inputs_follow_the_recipe(name):
    fx, inp = load_golden(f"metatree_lr_{name}.npz"), lro.case_inputs(CASE[name])
    for k, v in inp.items():
        assert np.array_equal(fx[k], v), k


@pytest.mark.parametrize("name", list(CASE))
def test_reference_is_within_its_own_yardstick_of_the_exact_state(name):
    """The fixture's exact tables against the reference's: post per column group within 4 x e_plain + 64 eps (+ D cond eps
    for mu), the rest as recorded in ref_vs_batch_*; and the conditioning the generator asserted."""
    fx, case = load_golden(f"metatree_lr_{name}.npz"), CASE[name]
    D = case["D"]
    for tag in ("1", "2"):
        exact = {k: fx[f"exact{tag}_{k}"] for k in orc.STATE}
        ref = {k: fx[f"after{tag}_{k}"] for k in orc.STATE}
        info = dict(s_beta=fx[f"exact{tag}_s_beta"], lam_scale=fx[f"exact{tag}_lam_scale"])
        visited = fx[f"exact{tag}_counts"] > 0
        e_plain = dict(zip(("lam", "beta", "mu", "cond"), fx[f"e_plain{tag}"]))
        errs = lro.post_errs(ref["post"], exact["post"], D, info, visited)
        bounds = lro.post_bounds(e_plain, D, errs["cond"])
        assert errs["n"] == 0 and errs["alpha"] == 0
        for k in ("lam", "beta", "mu"):
            assert errs[k] <= bounds[k], (name, tag, k, errs[k], bounds[k])
        assert errs["cond"] <= 1e3
        for v in np.flatnonzero(visited):
            assert info["s_beta"][v] / exact["post"][v, D + lro.tri(D) + 1] <= 10
        for k, e in lro.state_errs(ref, exact).items():
            assert e <= float(fx["ref_vs_batch_" + k]), (name, tag, k)


def test_exact_update_reproduces_the_fixture_s_exact_state():
    """One mpmath pass (the small three-way case): the oracle in the tree is the one the fixtures were made with."""
    fx, case = load_golden("metatree_lr_threeway.npz"), CASE["threeway"]
    D, flat = case["D"], {k: fx[k] for k in orc.STRUCT}
    st = lro.initial_state(flat, D, lro.default_h0(D), fx["init_g"], fx["init_prob"])
    for tag in ("1", "2"):
        before = st
        st, counts, info = lro.batch_update(flat, st, D, lro.default_h0(D), 2, fx["xc" + tag], fx["xk" + tag].astype(np.int64),
                                            fx["y" + tag])
        for k in orc.STATE:
            assert np.array_equal(st[k], fx[f"exact{tag}_{k}"], equal_nan=True), (tag, k)
        assert np.array_equal(counts, fx[f"exact{tag}_counts"])
        plain = lro.plain_update(flat, before, D, lro.default_h0(D), 2, fx["xc" + tag], fx["xk" + tag].astype(np.int64),
                                 fx["y" + tag])
        e = lro.post_errs(plain["post"], st["post"], D, info, counts > 0)
        assert max(e["lam"], e["beta"]) <= 64 * EPS and e["n"] == 0 and e["alpha"] == 0
        d = lro.decomposed_errs(flat, before, st, D, lro.default_h0(D), counts > 0)
        assert d["lml"] <= 2 * EPS and max(d["g"], d["lcm"], d["prob"]) <= 4 * EPS * d["scale"]
        assert lro.unchanged_where_unvisited(before, st, counts > 0)


@pytest.mark.parametrize("name", list(CASE))
def test_oracle_readouts_match_the_reference(name):
    fx, case = load_golden(f"metatree_lr_{name}.npz"), CASE[name]
    flat, st = {k: fx[k] for k in orc.STRUCT}, {k: fx["exact2_" + k] for k in orc.STATE}
    inp = {k: fx[k].astype(np.int64) if k.startswith("xk") else fx[k] for k in ("xcp", "xkp", "yp")}
    for k, v in lro.oracle_readouts(flat, st, case, inp).items():
        assert orc.rel_err(fx[k], v) <= float(fx["ref_vs_batch_" + k]) * (1 + 1e-9) + 4 * EPS, (name, k)


# ---- the model over the stand-in engine ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["threeway", "d15"])
def test_model_replays_the_fixture(mt, lr, name):
    """The fixture's forest handed to set_hn_params, both stages and every read-out through bayesml_amd.metatree."""
    fx, case = load_golden(f"metatree_lr_{name}.npz"), CASE[name]
    flat = {k: fx[k] for k in orc.STRUCT}
    inp = {k: fx[k].astype(np.int64) if k.startswith("xk") else fx[k] for k in fx if k[:2] in ("xc", "xk") or k[0] == "y"}
    out = lro.drive(mt, lr, case, inp, forest=(flat, fx["init_g"], fx["init_prob"]))
    for k in orc.STRUCT:
        assert np.array_equal(out[k], fx[k]), k
    for tag in ("1", "2"):
        for k in orc.STATE:                    # (the stand-in engine IS the exact oracle)
            assert np.array_equal(out[f"after{tag}_{k}"], fx[f"exact{tag}_{k}"], equal_nan=True), (tag, k)
    for k in ("predict", "pred_var", "pred_density"):
        assert orc.rel_err(out[k], fx[k]) <= 4 * float(fx["ref_vs_batch_" + k]) + 64 * EPS, k


def test_recorded_error_outcomes(mt, lr):
    with open(os.path.join(GOLDEN, "metatree_lr_errors.json")) as f:
        recorded = json.load(f)
    cases = lro.error_cases(mt, lr)
    assert sorted(cases) == sorted(recorded)
    for name, fn in cases.items():
        assert orc.outcome(fn) == recorded[name], name


def _fitted(mt, lr, sub_h0=None, n=60):
    sub_h0 = sub_h0 or {}
    case = lc.mixed_routing()
    m = mt.LearnModel(c_dim_continuous=2, c_dim_categorical=1, c_max_depth=4, c_num_children_vec=np.array([3, 2, 3]),
                      c_num_assignment_vec=np.array([1, -1, -1]), SubModel=lr, sub_constants={"c_degree": 2},
                      sub_h0_params=sub_h0)
    roots = orc.nodes_from_flat(mt, case["tabs"], case["state"]["g"], lambda: lr.LearnModel(2, **sub_h0))
    m.set_hn_params(hn_metatree_list=roots, hn_metatree_prob_vec=np.array([0.4, 0.6]))
    m.update_posterior(case["xc"][:n], case["xk"][:n], case["y"][:n], alg_type="given_MT")
    return m, case


def test_getters_setters_and_pickle(mt, lr):
    lam0 = np.array([[2.0, 0.5], [0.5, 3.0]])
    sub_h0 = dict(h0_mu_vec=np.array([0.5, -1.0]), h0_lambda_mat=lam0, h0_alpha=2.0, h0_beta=3.0)
    m, case = _fitted(mt, lr, sub_h0)
    assert np.array_equal(m._prior_vec(), lro.pack([0.5, -1.0], lam0, 2.0, 3.0, 0))
    trees = m.hn_metatree_list
    assert len(trees) == 2 and type(trees[0]) is mt._Node and type(trees[0].sub_model) is lr.LearnModel
    root = trees[0].sub_model
    assert root._n == 60 and root.hn_alpha == 2.0 + 30 and root.hn_lambda_mat.shape == (2, 2)
    assert np.array_equal(root.hn_lambda_mat, root.hn_lambda_mat.T) and np.array_equal(root.h0_lambda_mat, lam0)
    x = case["xc"][:60]
    assert np.allclose(root.hn_lambda_mat, lam0 + x.T @ x, rtol=1e-13)
    # an unvisited node keeps the prior, bit for bit
    few = _fitted(mt, lr, sub_h0, n=3)[0]
    st = few._engine.get_state()
    unseen = np.flatnonzero(np.isnan(st["lml"]))
    assert len(unseen) and all(np.array_equal(st["post"][v], few._prior_vec()) for v in unseen)
    assert all(t is None or isinstance(t, float) for t in (nd.log_marginal_likelihood for nd in few.hn_metatree_list[0].children))
    # the forest goes through set_hn_params and comes back unchanged
    before = m._hn_forest().state
    twin = mt.LearnModel(**{k: v for k, v in m.get_constants().items() if k != "sub_constants"}, SubModel=lr,
                         sub_constants={"c_degree": 2}, sub_h0_params=sub_h0)
    twin.set_hn_params(hn_metatree_list=trees, hn_metatree_prob_vec=m.hn_metatree_prob_vec)
    after = twin._hn_forest().state
    D, T = 2, 3
    for k in ("g", "prob"):
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(before["post"][:, :D + T + 2], after["post"][:, :D + T + 2])      # (_n is not a hyperparameter)
    # pickle: the tables survive, the engine does not
    m2 = pickle.loads(pickle.dumps(m))
    assert m2._engine is None and m2.SubModel is lr
    fk.use_cpu(m2)
    xp, kp = case["xc"][60:90], case["xk"][60:90]
    assert np.array_equal(m2.predict(xp, kp), m.predict(xp, kp))
    assert np.array_equal(m2.calc_pred_dist(xp, kp).calc_pred_var(), m.calc_pred_dist(xp, kp).calc_pred_var())
    params = m.get_hn_params()
    assert set(params) == {"hn_k_weight_vec", "hn_g", "sub_hn_params", "hn_metatree_list", "hn_metatree_prob_vec"}
    assert set(params["sub_hn_params"]) == {"hn_mu_vec", "hn_lambda_mat", "hn_alpha", "hn_beta"}
    m.estimate_params(visualize=False)
    assert m.calc_feature_importances().shape == (3,)


def test_sample_checks_follow_the_reference(mt, lr):
    from bayesml_amd._exceptions import DataFormatError, ParameterFormatError
    m, case = _fitted(mt, lr)
    xc, xk, y = case["xc"][:20], case["xk"][:20], case["y"][:20]
    before = m._engine.get_state()
    with pytest.raises(DataFormatError, match="x.shape\\[:-1\\] and y.shape must be same"):
        m.update_posterior(xc, xk, y[:5], alg_type="given_MT")
    with pytest.raises(DataFormatError):
        m.update_posterior(xc, xk, y[:, None], alg_type="given_MT")
    with pytest.raises(ParameterFormatError):
        m.update_posterior(xc[:, :1], xk, y, alg_type="given_MT")
    with pytest.raises(DataFormatError):
        m.update_posterior(xc, xk, ["a"] * 20, alg_type="given_MT")
    after = m._engine.get_state()
    assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)
    m.update_posterior(xc, xk, np.arange(20), alg_type="given_MT")           # integers are cast, as in the reference
    dens = m.calc_pred_dist(xc, xk).calc_pred_density(y)
    assert dens.shape == (20,) and np.all(dens > 0)
    want = lro.pred_density(case["tabs"], m._engine.get_state(), 2, 2, xc, xk, y)
    assert np.allclose(dens, want, rtol=1e-12)


def test_mtrf_on_the_stand_in(mt, lr):
    pytest.importorskip("sklearn")
    x, y = lc.sample(300, 3, seed=23)
    m = mt.LearnModel(3, 0, c_max_depth=2, SubModel=lr, sub_constants={"c_degree": 3})
    m.fit(x, None, y, n_estimators=3, random_state=0)
    assert all(t.sub_model._n == 300 for t in m.hn_metatree_list)
    assert np.sqrt(np.mean((m.predict(x, None) - y) ** 2)) < 1.2


def test_seeded_genmodel_fixture(mt, lr):
    fx = load_golden("metatree_lr_gen.npz")
    for name, kw in (("even", {}), ("random", dict(threshold_type="random"))):
        m = mt.GenModel(2, 1, c_max_depth=3, c_num_children_vec=np.array([2, 3, 2]), SubModel=lr,
                        sub_constants={"c_degree": 2}, h_g=0.75, seed=7)
        m.gen_params(**kw)
        flat = orc.flatten_gen(m.root)
        for k in ("feat", "nchild", "depth"):
            assert np.array_equal(flat[k], fx[f"{name}_{k}"]), (name, k)
        for k in ("thr", "g", "params"):
            assert np.allclose(flat[k], fx[f"{name}_{k}"], rtol=1e-13, atol=0, equal_nan=True), (name, k)
        xc, xk, y = m.gen_sample(40)
        assert np.array_equal(xk, fx[f"{name}_xk"])
        assert np.allclose(xc, fx[f"{name}_xc"], rtol=1e-13) and np.allclose(y, fx[f"{name}_y"], rtol=1e-12, atol=1e-13)
    assert type(m.root.sub_model) is lr.GenModel and m.get_constants()["sub_constants"] == {"c_degree": 2}


# ---- the edge cases reach what they name --------------------------------------------------------------------------------------
def test_edge_cases_reach_what_they_name():
    from bayesml_amd import _mtree
    B = _mtree.LR_BLOCK
    for kind, sizes in (("crossing", (B + 5, 37)), ("ending", (B, 37)), ("three_blocks", (2 * B + 3, 10))):
        case, got = lc.block_edge(kind, B)
        stops = orc.stops(orc.route(case["tabs"], 3, case["xc"], None))[0]
        assert got == sizes and (np.count_nonzero(stops == 1), np.count_nonzero(stops == 2)) == sizes
    case = lc.scattered(B)
    stops = orc.stops(orc.route(case["tabs"], 3, case["xc"], None))[0]
    assert len(stops) > 3 * B and _mtree.slabs_for(len(stops), 3, 1) >= 3
    assert np.count_nonzero(np.diff(stops)) > len(stops) // 4                 # the leaves alternate through the batch
    case = lc.tiny_runs()
    stops = orc.stops(orc.route(case["tabs"], 2, case["xc"], None))[0]
    leaves = np.flatnonzero(case["tabs"]["feat"] < 0)
    sizes = np.array([np.count_nonzero(stops == v) for v in leaves])
    assert len(leaves) == 16 and (sizes == 0).any() and (sizes > 0).sum() >= 8 and sizes.max() < 16
    case = lc.precision_edge()
    conds = [np.linalg.cond(np.eye(3) + case["xc"][m].T @ case["xc"][m]) for m in (case["xc"][:, 0] < 0, case["xc"][:, 0] >= 0)]
    assert all(1e4 <= c <= 1e5 for c in conds), conds
    case = lc.mixed_routing()
    assert sorted(set(case["tabs"]["nchild"])) == [0, 2, 3] and case["dim_cat"] == 1
    for n in (1, 3, 4, 5):
        assert lc.quad_padding(n)["xc"].shape == (n, 1)
    assert lc.tile_edge(15, np.float32)["xc"].dtype == np.float32
