"""metatree without a GPU: the exact oracle against the reference's fixtures, every LearnModel / GenModel method through the
NumPy stand-in engine (tests/fake_metatree_engine.py) against the fixtures and the recorded boundary outcomes, and the
mtree_* argument checks of the library."""
import ctypes
import json
import os
import pickle
import warnings

import numpy as np
import pytest

import fake_metatree_engine as fk
import metatree_edge_cases as ec
import metatree_oracle as orc
from conftest import GOLDEN, load_golden

EPS = np.finfo(float).eps
NAMES = [c["name"] for c in orc.CASES]
CASE = {c["name"]: c for c in orc.CASES}


def _subs():
    from bayesml_amd import bernoulli, categorical, exponential, normal, poisson
    return dict(bernoulli=bernoulli, categorical=categorical, poisson=poisson, exponential=exponential, normal=normal)


@pytest.fixture()
def mt():
    from bayesml_amd import metatree
    fk.use_cpu(metatree.LearnModel)
    yield metatree
    metatree.LearnModel._mtree_pass_factory = None


def test_package_exports_metatree():
    import bayesml_amd
    for name in ("metatree", "linearregression", "autoregressive"):
        assert name in bayesml_amd.__all__ and hasattr(bayesml_amd, name)
    assert {"GenModel", "LearnModel"} <= set(bayesml_amd.metatree.__all__)
    assert bayesml_amd.metatree.LearnModel._mtree_pass_factory is None


@pytest.mark.parametrize("name", NAMES)
def test_fixture_inputs_follow_the_recipe(name):
    fx, inp = load_golden(f"metatree_{name}.npz"), orc.case_inputs(CASE[name])
    for k, v in inp.items():
        assert np.array_equal(fx[k], v), k


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_fixtures(name):
    """The exact batch form from the stored forest and prior state: within the recorded ref_vs_batch of the reference at
    both stages (counts and integer columns exactly), and the oracle's read-outs on that state within theirs."""
    fx, case = load_golden(f"metatree_{name}.npz"), CASE[name]
    fam, dc = orc.FAMILY[case["sub"]], case["consts"]["c_dim_continuous"]
    degree = case.get("sub_constants", {}).get("c_degree", 0)
    h0 = orc.post_of(fam, _subs()[case["sub"]].LearnModel(**case.get("sub_constants", {})))
    flat = {k: fx[k] for k in orc.STRUCT}
    n = len(flat["feat"])
    st = dict(g=fx["init_g"], post=np.tile(h0, (n, 1)), lml=np.full(n, np.nan), lcm=np.zeros(n), prob=fx["init_prob"])
    for stage, tag in (("after1", "1"), ("after2", "2")):
        st, _ = orc.batch_update(flat, st, fam, degree, h0, dc, fx["xc" + tag], fx["xk" + tag], fx["y" + tag])
        errs = orc.state_errs({k: fx[f"{stage}_{k}"] for k in orc.STATE}, st)
        for k, e in errs.items():
            assert e <= float(fx["ref_vs_batch_" + k]), (stage, k, e)
        if fam in (orc.BERNOULLI, orc.CATEGORICAL):
            assert np.array_equal(st["post"], fx[f"{stage}_post"])
        assert orc.fixed_points_kept(fx["init_g"], st["g"])
    for k, v in orc.oracle_readouts(flat, st, case, {k: fx[k] for k in ("xcp", "xkp", "yp")}).items():
        assert orc.rel_err(fx[k], v) <= float(fx["ref_vs_batch_" + k]), k


@pytest.mark.parametrize("name", NAMES)
def test_learnmodel_against_fixtures(mt, name):
    """Every stage and read-out of the case through LearnModel on the stand-in, replayed from the stored forest."""
    fx, case = load_golden(f"metatree_{name}.npz"), CASE[name]
    forest = ({k: fx[k] for k in orc.STRUCT}, fx["init_g"], fx["init_prob"])
    out = orc.drive(mt, _subs(), case, orc.case_inputs(case), forest=forest)
    tol = {k: 4 * float(fx["ref_vs_batch_" + k]) + 64 * EPS for k in ("g", "post", "lml", "prob")}
    for k in orc.STRUCT:
        assert np.array_equal(out[k], fx[k]), k
    for stage in ("after1", "after2"):
        errs = orc.state_errs({k: out[f"{stage}_{k}"] for k in orc.STATE}, {k: fx[f"{stage}_{k}"] for k in orc.STATE})
        for k, e in errs.items():
            assert e <= tol[k], (stage, k, e)
        assert orc.rel_err(out[f"{stage}_lcm"], fx[f"{stage}_lcm"]) <= tol["lml"]
    read = orc.readout_tols(fx)
    for k in orc.READOUTS:
        if k in fx and np.asarray(fx[k]).dtype.kind == "f":
            assert orc.rel_err(out[k], fx[k]) <= read[k], k
    if out["predict"].dtype.kind != "f":
        top = np.sort(fx["predict_proba"], axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * read["predict_proba"]
        assert clear.mean() > 0.9 and np.array_equal(out["predict"][clear], fx["predict"][clear])
    assert int(out["map_index"]) == int(fx["map_index"]) and np.array_equal(out["map_leaf"], fx["map_leaf"])


def test_boundary_outcomes(mt):
    with open(os.path.join(GOLDEN, "metatree_errors.json")) as f:
        want = json.load(f)
    got = {name: orc.outcome(fn) for name, fn in orc.error_cases(mt, _subs()).items()}
    assert got == want


def test_bad_categorical_changes_nothing(mt):
    from bayesml_amd import DataFormatError
    case = CASE["threeway"]
    inp = orc.case_inputs(case)
    flat, g = orc._hand_forest()
    m = mt.LearnModel(SubModel=_subs()["bernoulli"], **orc._HAND)
    m.set_hn_params(hn_metatree_list=orc.nodes_from_flat(mt, flat, g, _subs()["bernoulli"].LearnModel))
    m.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    before = {k: np.array(v) for k, v in m._hn_forest().state.items()}
    import torch
    bad = torch.from_numpy(inp["xk2"].copy())          # (a tensor: the host pre-check leaves its values to the engine)
    bad[3, 0] = 3
    with pytest.raises(DataFormatError, match=r"x_categorical\[:,0\].max\(\) must smaller than"):
        m.update_posterior(torch.from_numpy(inp["xc2"]), bad, torch.from_numpy(inp["y2"]), alg_type="given_MT")
    for k, v in m._hn_forest().state.items():
        assert np.array_equal(v, before[k], equal_nan=True), k


def test_pred_and_update_get_p_params_and_mtrf_refusal(mt):
    """pred_and_update = the prediction from the state before, then a 'given_MT' update on the same rows (every loss the
    family has); get_p_params is None as in the reference; a sample MTRF refuses leaves the posterior forest as it was,
    whatever holds the sample."""
    import torch
    from bayesml_amd import CriteriaError, DataFormatError
    inp = orc.case_inputs(CASE["threeway"])
    flat, g = orc._hand_forest()

    def model(sub_name, **kw):
        sub = _subs()[sub_name]
        m = mt.LearnModel(SubModel=sub, **{**orc._HAND, **kw})
        return m.set_hn_params(hn_metatree_list=orc.nodes_from_flat(mt, flat, g, sub.LearnModel))

    for loss, read in (("KL", lambda m: m.predict_proba(inp["xc2"], inp["xk2"])), ("0-1", lambda m: m.predict(inp["xc2"], inp["xk2"])),
                       (None, lambda m: m.predict(inp["xc2"], inp["xk2"]))):
        a, b = model("bernoulli"), model("bernoulli")
        for m in (a, b):
            m.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
        want = read(b)
        b.update_posterior(inp["xc2"], inp["xk2"], inp["y2"], alg_type="given_MT")
        assert np.array_equal(a.pred_and_update(inp["xc2"], inp["xk2"], inp["y2"], loss=loss), want)
        for k in orc.STATE:
            assert np.array_equal(a._hn_forest().state[k], b._hn_forest().state[k], equal_nan=True), (loss, k)
    with pytest.raises(CriteriaError):
        a.pred_and_update(inp["xc2"], inp["xk2"], inp["y2"], loss="squared")
    assert a.get_p_params() is None
    # MTRF on a binary model: the bad value is found before scikit-learn runs and before the forest is replaced
    m = mt.LearnModel(2, 1)
    x, k, y = inp["xc1"], inp["xk1"] % 2, inp["y1"]
    for bad in (np.where(np.arange(len(k))[:, None] == 5, 2, k), torch.from_numpy(np.where(np.arange(len(k))[:, None] == 5, 2, k))):
        with pytest.raises(DataFormatError, match="must smaller than"):
            m.update_posterior(x, bad, y, alg_type="MTRF", n_estimators=2)
        assert m._hn is None and m.hn_metatree_list == []
    with pytest.raises(DataFormatError):
        a.calc_pred_dist(inp["xcp"], torch.from_numpy(inp["xkp"]) - 1)


def test_genmodel_save_sample(mt, tmp_path):
    g = mt.GenModel(2, 1, seed=5).gen_params()
    g.save_sample(str(tmp_path / "s"), 7)
    twin = mt.GenModel(2, 1, seed=5).gen_params()
    with np.load(tmp_path / "s.npz") as z:
        for got, want in zip((z["x_continuous"], z["x_categorical"], z["y"]), twin.gen_sample(7)):
            assert np.array_equal(got, want)
        assert z["x_continuous"].shape == (7, 2) and z["x_categorical"].shape == (7, 1) and z["y"].shape == (7,)


def test_out_of_scope_items_name_themselves(mt):
    from bayesml_amd import linearregression
    from bayesml_amd._engine import EngineLimitError
    with pytest.raises(EngineLimitError, match="linearregression"):
        mt.LearnModel(2, 0, SubModel=linearregression)
    with pytest.raises(EngineLimitError, match="linearregression"):
        mt.GenModel(2, 0, SubModel=linearregression)
    m = mt.LearnModel(2, 0)
    x, y = np.zeros((4, 2)), np.zeros(4, dtype=int)
    for alg in ("MTMCMC", "REMTMCMC"):
        with pytest.raises(NotImplementedError, match=alg):
            m.update_posterior(x, None, y, alg_type=alg)
    for call in (m.visualize_posterior, lambda: m.estimate_params(visualize=True), mt.GenModel(2, 0).visualize_model):
        with pytest.raises(NotImplementedError, match="plotting"):
            call()
    with pytest.raises(EngineLimitError, match="bayesml itself has no such limit"):
        mt.LearnModel(1, 1, c_num_children_vec=np.array([2, 17]))


def test_mtrf_equals_given_mt_on_its_forest(mt):
    """MTRF end to end: the forest scikit-learn grows is copied (leaves h_g = 0, thresholds between the range ends,
    k_candidates shrinking under c_num_assignment_vec), merged and updated; the same forest handed back with 'given_MT'
    gives the same posterior."""
    pytest.importorskip("sklearn")
    case = dict(CASE["normal"], consts=dict(CASE["normal"]["consts"], c_num_assignment_vec=np.array([4, -1, -1, 4, -1])))
    inp, sub = orc.case_inputs(case), _subs()["normal"]
    a = mt.LearnModel(SubModel=sub, **case["consts"])
    a.fit(inp["xc1"][:500], inp["xk1"][:500], inp["y1"][:500], n_estimators=6, random_state=1)
    fa, sa, _ = orc.flatten(a.hn_metatree_list, a.hn_metatree_prob_vec, orc.NORMAL)
    assert len(fa["tree_off"]) - 1 <= 6 and fa["depth"].max() <= 4 and np.all(sa["g"][fa["feat"] < 0] == 0.0)
    for root in a.hn_metatree_list:                    # a feature with a bounded number of assignments is used up by its use
        stack = [root]
        while stack:
            node = stack.pop()
            assert node.leaf or node.k in node.k_candidates
            if not node.leaf:
                assert node.k >= 3 or node.ranges[node.k, 0] <= node.thresholds[1] <= node.ranges[node.k, 1]
                if node.k in (0, 3):
                    assert all(c.k_candidates.count(node.k) == node.k_candidates.count(node.k) - 1 for c in node.children)
                stack.extend(node.children)
    b = mt.LearnModel(SubModel=sub, **case["consts"])
    trees = a._mtrf(inp["xc1"][:500], inp["xk1"][:500], inp["y1"][:500], n_estimators=6, random_state=1)
    b._set_hn(trees)
    b.update_posterior(inp["xc1"][:500], inp["xk1"][:500], inp["y1"][:500], alg_type="given_MT")
    _, sb, _ = orc.flatten(b.hn_metatree_list, b.hn_metatree_prob_vec, orc.NORMAL)
    for k in orc.STATE:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), k


def test_forest_round_trips(mt):
    """A _Node forest through the setters and getters, h0 -> hn, overwrite_h0_params, and pickling."""
    sub = _subs()["poisson"]
    flat, g = orc._hand_forest()
    m = mt.LearnModel(SubModel=sub, h0_g=0.25, sub_h0_params={"h0_alpha": 2.0}, **orc._HAND)
    assert m.hn_metatree_list == [] and m.hn_metatree_prob_vec is None
    m.set_h0_params(h0_metatree_list=orc.nodes_from_flat(mt, flat, g, sub.LearnModel),
                    h0_metatree_prob_vec=np.array([0.25, 0.75]))
    for which in ("h0", "hn"):
        params = getattr(m, f"get_{which}_params")()
        assert list(params) == [f"{which}_k_weight_vec", f"{which}_g", f"sub_{which}_params", f"{which}_metatree_list",
                                f"{which}_metatree_prob_vec"]
        f2, s2, _ = orc.flatten(params[f"{which}_metatree_list"], params[f"{which}_metatree_prob_vec"], orc.POISSON)
        for k in orc.STRUCT:
            assert np.array_equal(f2[k], flat[k]), (which, k)
        assert np.array_equal(s2["g"], g) and np.array_equal(s2["prob"], [0.25, 0.75])
        assert np.all(np.isnan(s2["lml"]))
    root = m.hn_metatree_list[0]
    assert root.k_candidates == [0, 1, 2] and root.children[1].k_candidates == [1, 2]       # c_num_assignment_vec = [1, -1, -1]
    assert np.array_equal(root.children[1].ranges, [[-1.0, 1.0], [-3.0, 3.0]]) and root.log_marginal_likelihood is None
    inp = orc.case_inputs(CASE["threeway_n1"])
    m.set_hn_params(hn_g=0.6)
    assert m.hn_metatree_list[0].h_g == 0.6 and m.hn_metatree_list[0].children[1].children[0].h_g == 0.0
    m.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    m2 = pickle.loads(pickle.dumps(m))
    for k, v in m._hn_forest().state.items():
        assert np.array_equal(v, m2._hn_forest().state[k], equal_nan=True), k
    assert np.array_equal(m.predict(inp["xcp"], inp["xkp"]), m2.predict(inp["xcp"], inp["xkp"]))
    m.overwrite_h0_params()
    # (ref:1301-1306: the copy reads a LearnModel node's h0, so structure and h_g come over and the sub-models' prior stays)
    assert m.h0_metatree_list[0].sub_model.h0_alpha == 2.0 and m.h0_metatree_list[0].h_g == m2.hn_metatree_list[0].h_g
    with pytest.raises(Exception, match="must be a list"):
        m.set_hn_params(hn_metatree_list=root)
    with pytest.raises(Exception, match="must be the same"):
        m.set_hn_params(hn_metatree_prob_vec=np.array([1.0]))


def test_genmodel_follows_the_reference_draws(mt):
    """gen_params and gen_sample under a seed: structure and integers exactly, floats to the last digit but one (the
    expfam_*_gen fixtures' rule: 4 eps relative)."""
    fx = load_golden("metatree_gen.npz")
    subs = _subs()
    for name, sub, kw in (("bern", subs["bernoulli"], {}), ("norm", subs["normal"], dict(threshold_type="random"))):
        m = mt.GenModel(2, 1, c_max_depth=3, c_num_children_vec=np.array([2, 3, 2]), SubModel=sub, h_g=0.75, seed=7)
        m.gen_params(**kw)
        flat = orc.flatten_gen(m.root)
        for k in ("feat", "nchild", "depth"):
            assert np.array_equal(flat[k], fx[f"{name}_{k}"]), (name, k)
        for k in ("thr", "g", "params"):
            assert np.allclose(flat[k], fx[f"{name}_{k}"], rtol=4 * EPS, atol=0, equal_nan=True), (name, k)
        xc, xk, y = m.gen_sample(40)
        assert np.array_equal(xk, fx[f"{name}_xk"]) and np.allclose(xc, fx[f"{name}_xc"], rtol=4 * EPS, atol=0)
        if y.dtype.kind == "i":
            assert np.array_equal(y, fx[f"{name}_y"])
        else:
            assert np.allclose(y, fx[f"{name}_y"], rtol=4 * EPS, atol=0)
    g = mt.GenModel(2, 1, seed=3)
    assert list(g.get_constants()) == ["c_dim_continuous", "c_dim_categorical", "c_num_children_vec", "c_max_depth",
                                       "c_num_assignment_vec", "c_ranges", "sub_constants"]
    assert list(g.get_h_params()) == ["h_k_weight_vec", "h_g", "sub_h_params", "h_metatree_list", "h_metatree_prob_vec"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g.gen_params(feature_fix=True).gen_params(feature_fix=True, tree_fix=True)
    h = mt.GenModel(2, 1, seed=4).set_params(g.get_params()["root"])
    assert orc.flatten_gen(h.root)["feat"].tolist() == orc.flatten_gen(g.root)["feat"].tolist()
    x_c, x_k, y = h.gen_sample(x_continuous=np.zeros((5, 2)))
    assert x_k.shape == (5, 1) and y.shape == (5,)


# ---- the library's argument checks (no GPU) ----------------------------------------------------------------------------------
def _struct(**kw):
    from bayesml_amd import _mtree
    base = dict(n_trees=1, n_nodes=3, n_thr=3, max_tree_nodes=3, max_children=2, max_depth=1, dim_cont=1, dim_cat=0,
                tree_off_dev=64, feat_dev=64, child0_dev=64, nchild_dev=64, thr_off_dev=64, depth_dev=64, thr_dev=64)
    base.update(kw)
    return _mtree.ForestStruct(**base)


def test_mtree_argument_checks_without_gpu():
    from bayesml_amd import _mtree
    lib = _mtree.load_library()
    assert lib.mtree_abi_version() == 2
    ni, nr, npost = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for fam in range(5):
        assert lib.mtree_stat_cols(fam, 3, ni, nr, npost) == 0
        assert (ni.value, nr.value, npost.value) == _mtree.stat_cols(fam, 3)
    assert lib.mtree_stat_cols(7, 0, ni, nr, npost) == 1 and lib.mtree_stat_cols(_mtree.CATEGORICAL, 17, ni, nr, npost) == 2
    assert lib.mtree_work_len(10, _mtree.NORMAL, 0, 4) == 10 * (1 + 4 * 2) and lib.mtree_work_len(10, 0, 0, 65) == -1
    ok = _struct()
    route = lambda f, n=8, stop=64, bad=64, xc=64, dt=_mtree.F64: lib.mtree_route(      # noqa: E731
        ctypes.byref(f), dt, xc, _mtree.U8, None, None, n, stop, None, bad, None)
    # (every call below is refused before anything touches the device: the pointers are made-up addresses)
    assert route(ok, n=0) == 1 and b"n must be >= 1" in lib.mtree_last_error()
    assert route(ok, stop=None) == 1 and route(ok, xc=None) == 1 and route(ok, dt=_mtree.U8) == 1
    assert route(ok, xc=68) == 1 and b"aligned" in lib.mtree_last_error()
    assert route(_struct(n_trees=0)) == 1 and route(_struct(feat_dev=None)) == 1 and route(_struct(thr_dev=68)) == 1
    for over in (dict(n_trees=1025, n_nodes=2000), dict(max_tree_nodes=4097, n_nodes=5000), dict(max_children=17),
                 dict(max_depth=25)):
        assert route(_struct(**over)) == 2 and b"not supported" in lib.mtree_last_error()
    assert lib.mtree_reduce(ctypes.byref(ok), 0, 0, 64, 64, 8, 0, 64, 64, 64, None) == 1
    assert lib.mtree_reduce(ctypes.byref(ok), 0, 0, 64, None, 8, 1, 64, 64, 64, None) == 1
    assert lib.mtree_reduce(ctypes.byref(ok), 1, 17, 64, 64, 8, 1, 64, 64, 64, None) == 2
    assert lib.mtree_sweep(ctypes.byref(ok), 0, 0, 64, 64, None, 64, 64, 64, 64, 64, 64, None) == 1
    assert lib.mtree_predict(ctypes.byref(ok), _mtree.BERNOULLI, 0, _mtree.PRED_MEAN, _mtree.F64, 64, 0, None, 8, 64, 64, 64,
                             64, 64, None) == 1 and b"no such read-out" in lib.mtree_last_error()
    assert lib.mtree_predict(ctypes.byref(ok), _mtree.POISSON, 0, _mtree.PRED_VAR, _mtree.F64, 64, 0, None, 8, 64, 64, 64, 64,
                             64, None) == 1
    assert lib.mtree_predict(ctypes.byref(ok), _mtree.NORMAL, 0, 9, _mtree.F64, 64, 0, None, 8, 64, 64, 64, 64, 64, None) == 1


def test_limits_raise_engine_limit_error():
    from bayesml_amd import _mtree
    from bayesml_amd._engine import EngineLimitError
    _mtree.check_limits(1024, 2047, 2, 10)           # binary trees of depth 10 and 1024 trees fit
    for args in ((1025, 10, 2, 3), (1, 4097, 2, 3), (1, 10, 17, 3), (1, 10, 2, 25), (1, 10, 2, 3, 17)):
        with pytest.raises(EngineLimitError, match="bayesml itself has no such limit"):
            _mtree.check_limits(*args)
    assert _mtree.slabs_for(1, 100, 2) == 1 and _mtree.slabs_for(1025, 100, 2) == 2 and _mtree.slabs_for(10 ** 7, 100, 2) == 64
    assert _mtree.slabs_for(10 ** 7, 1024 * 2047, 3) == 10


def test_there_is_no_cpu_fallback():
    from bayesml_amd import metatree
    from bayesml_amd._engine import EngineUnavailableError
    assert metatree.LearnModel._mtree_pass_factory is None
    flat, g = orc._hand_forest()
    sub = _subs()["bernoulli"]
    m = metatree.LearnModel(SubModel=sub, device="cpu", **orc._HAND)          # (refused with or without a GPU in the box)
    m.set_hn_params(hn_metatree_list=orc.nodes_from_flat(metatree, flat, g, sub.LearnModel))      # host only
    inp = orc.case_inputs(CASE["threeway"])
    with pytest.raises(EngineUnavailableError):
        m.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")


# ---- the yardsticks of tests/test_gpu_metatree_edges.py, pinned without a GPU ------------------------------------------------
def _fixture_start(name):
    fx, case = load_golden(f"metatree_{name}.npz"), CASE[name]
    fam, dc = orc.FAMILY[case["sub"]], case["consts"]["c_dim_continuous"]
    degree = case.get("sub_constants", {}).get("c_degree", 0)
    h0 = orc.post_of(fam, _subs()[case["sub"]].LearnModel(**case.get("sub_constants", {})))
    flat = {k: fx[k] for k in orc.STRUCT}
    n = len(flat["feat"])
    st = dict(g=fx["init_g"], post=np.tile(h0, (n, 1)), lml=np.full(n, np.nan), lcm=np.zeros(n), prob=fx["init_prob"])
    return fx, flat, st, fam, degree, h0, dc


@pytest.mark.parametrize("name", NAMES)
def test_plain_update_is_the_references_arithmetic(name):
    """``plain_update`` (per node, float64 numpy) reproduces the reference's own first-stage state within 64 eps in the
    existing metrics, and ``node_errs`` of a state against itself is 0."""
    fx, flat, st, fam, degree, h0, dc = _fixture_start(name)
    plain = orc.plain_update(flat, st, fam, degree, h0, dc, fx["xc1"], fx["xk1"], fx["y1"])
    errs = orc.state_errs(plain, {k: fx[f"after1_{k}"] for k in orc.STATE})
    assert max(errs.values()) <= 64 * EPS and orc.rel_err(plain["lcm"], fx["after1_lcm"]) <= 64 * EPS, errs
    scales = orc.m_scales(flat, st, dc, fx["xc1"], fx["xk1"], fx["y1"]) if fam == orc.NORMAL else None
    assert not orc.node_errs(fam, fx["after1_post"], fx["after1_post"], scales).any()
    # the fixture's own state is within 4 x e_plain + 64 eps of the exact one, per node and column (it IS the plain form)
    exact, _ = orc.batch_update(flat, st, fam, degree, h0, dc, fx["xc1"], fx["xk1"], fx["y1"])
    e, bound = orc.node_errs(fam, fx["after1_post"], exact["post"], scales), orc.post_bounds(fam, plain["post"], exact["post"], scales)
    for c in range(e.shape[1]):
        assert e[:, c].max() <= bound.get(c, 0.0), (c, e[:, c].max())


def test_node_errs_sees_one_small_node_beside_a_large_one():
    """What the array-wide metric hides: a level of 1e6 in one node's m allows 1e-8 on every beta; per node it does not."""
    want = np.array([[1e6, 11.0, 6.0, 3.0, 10.0], [0.5, 3.0, 2.0, 1e-3, 2.0]])
    got = want.copy()
    got[1, 3] += 1e-9
    assert orc.rel_err(got, want) <= 64 * EPS
    e = orc.node_errs(orc.NORMAL, got, want, scales=[1e6, 0.5])
    assert e[1, 3] > 1e-7 and e[0].max() == 0 and e[1, [0, 1, 2, 4]].max() == 0
    got[0, 1] = np.nextafter(11.0, 12.0)
    assert np.isinf(orc.node_errs(orc.NORMAL, got, want, scales=[1e6, 0.5])[0, 1])
    got = want.copy()
    got[0, 0] += 1e-6
    assert orc.node_errs(orc.NORMAL, got, want, scales=[1e6, 0.5])[0, 0] == pytest.approx(1e-12, rel=1e-3)


def test_predict_ld_agrees_with_predict():
    """The long-double fold rounded to float64 agrees with the float64 oracle to a few eps on the fixtures' states: e64, the
    unit of the prediction bounds, is the float64 fold's own rounding and nothing else."""
    for name, mode in (("bernoulli", "proba"), ("poisson", "mean"), ("normal", "var")):
        fx, flat, _, fam, degree, _, dc = _fixture_start(name)
        st = {k: fx[f"after2_{k}"] for k in orc.STATE}
        f64 = orc.predict(flat, st, fam, degree, dc, fx["xcp"], fx["xkp"], mode)
        ld = orc.predict_ld(flat, st, fam, degree, dc, fx["xcp"], fx["xkp"], mode)
        assert ld.dtype == np.longdouble and ld.shape == f64.shape
        e64 = orc.entry_err(f64, ld)
        assert e64.max() <= (64 if mode != "var" else 4096) * EPS, (name, e64.max())
        assert np.all(np.abs(ld.astype(np.float64) - f64) <= e64 * np.abs(f64) + np.spacing(f64))


def _exact(case, state=None):
    return orc.batch_update(case["tabs"], case["state"] if state is None else state, case["fam"], case["degree"], case["h0"],
                            case["dim_cont"], case["xc"], case["xk"], case["y"])


def _inner_seen(case, want):
    return (case["tabs"]["feat"] >= 0) & ~np.isnan(want["lml"])


def test_edge_cases_reach_what_they_name():
    """Every claim of tests/metatree_edge_cases.py, so that no GPU test passes on a case that misses its branch."""
    from bayesml_amd import _mtree
    assert (ec.LDS_SLOTS, ec.MAX_SLABS, ec.MIN_SPAN) == (_mtree.LDS_SLOTS, _mtree.MAX_SLABS, _mtree.MIN_SPAN)
    # conditioning (post alone is judged there): the recipes hold what their names say
    for kind in ec.CONDITIONING:
        for fam in (orc.NORMAL, orc.EXPONENTIAL):
            for seed, n in ((0, 200), (1, 200), (10, 50), (11, 50)):
                case = ec.conditioning(kind, fam, n=n, seed=seed)
                leaf = case["claims"]["leaf"]
                assert (case["y"] > 0).all() or fam == orc.NORMAL
                if kind.startswith("outlier"):
                    assert (leaf == 0).sum() == 1 and leaf[0] == 0 and case["y"][0] == float(kind.split("_")[1])
                    assert np.all(np.abs(case["y"][1:] - 1e-3) < 1e-3)
                if kind == "constant":
                    assert (leaf == 3).sum() >= 3 and len(set(case["y"][leaf == 3])) == 1
                if kind == "scales" and n == 200:
                    assert len(set(leaf)) == 8 and case["y"].max() / np.abs(case["y"]).min() > 1e20
        _, counts = _exact(ec.conditioning(kind, orc.NORMAL))
        assert counts[0] == 200 and (counts[:7] > 0).all()
    # own rows at inner nodes
    for fam in (orc.NORMAL, orc.EXPONENTIAL, orc.POISSON):
        case = ec.nan_rows(fam)
        want, counts = _exact(case)
        assert case["claims"]["own_root"] > 0 and case["claims"]["own_d1"] > 0
        assert counts[0] - counts[1] - counts[2] == case["claims"]["own_root"]
        assert counts[1] - counts[3] - counts[4] > 0 and counts[2] - counts[5] - counts[6] > 0
        inner = _inner_seen(case, want)
        # (the root's children do not hold its own rows, so their L sum is far above its lml and its h_g ends next to 1)
        assert inner.sum() == 7 and np.all((want["g"][1:7] > 0) & (want["g"][1:7] < 1)) and want["g"][0] > 0.5
    # the mixture: t = ln(1 - g0) + lml - ln g0 - sum L of node 1 is beyond exp's range for every g0 inside (0, 1)
    mp = orc.mp
    for fam in (orc.BERNOULLI, orc.NORMAL):
        for sign in (-1, 1):
            want, _ = _exact(ec.mixture(fam, 0.5, sign))
            gap = mp.mpf(float(want["lml"][1])) - mp.mpf(float(want["lcm"][3])) - mp.mpf(float(want["lcm"][4]))
            for g0 in ec.G0[2:]:
                t = mp.log(1 - mp.mpf(g0)) - mp.log(mp.mpf(g0)) + gap
                assert sign * t > 1000, (fam, sign, g0, t)
            assert want["prob"][1] == 0.0 and want["prob"][2] == 0.0 and 1e-3 < want["prob"][3] < 0.999
    assert len(set(ec.G0)) == 7 and {0.0, 1.0, 5e-324, 1e-300, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53} == set(ec.G0)
    # limits
    case = ec.wide_continuous()
    paths = orc.route(case["tabs"], 1, case["xc"], None)
    stops = orc.stops(paths)[0]
    assert set(stops) == set(range(17)) and (stops == 0).sum() == 1           # every child, and the NaN row at the root
    x = case["xc"][:, 0]
    assert np.array_equal(stops[:17], np.minimum(np.arange(17), 15) + 1) and stops[x == -np.inf] == 1 and stops[x == np.inf] == 16
    assert np.array_equal(case["xc"].astype(np.float32).astype(np.float64), case["xc"], equal_nan=True)
    for card in (16, 20):
        case = ec.wide_categorical(card)
        assert case["claims"]["outside"] == (0 if card == 16 else (case["xk"] >= 16).sum()) and set(case["xk"][:, 0]) == set(range(card))
    for fam, degree, n_nodes, lds in ((orc.CATEGORICAL, 16, 361, True), (orc.CATEGORICAL, 16, 362, False),
                                      (orc.POISSON, 0, 2048, True), (orc.POISSON, 0, 2049, False)):
        case = ec.lds_edge(fam, n_nodes, degree)
        tabs = case["tabs"]
        slots = n_nodes * case["claims"]["cols"]
        assert len(tabs["feat"]) == n_nodes and case["claims"]["lds"] == lds == (slots <= _mtree.LDS_SLOTS)
        assert slots == {361: 6137, 362: 6154, 2048: 6144, 2049: 6147}[n_nodes]
        assert np.all(np.diff(tabs["depth"]) >= 0) and np.all(tabs["child0"][tabs["feat"] >= 0] > np.flatnonzero(tabs["feat"] >= 0))
        assert (orc.stops(orc.route(tabs, 1, case["xc"], None))[0] == n_nodes - 1).sum() >= 40
        _mtree.check_limits(1, n_nodes, 2, int(tabs["depth"].max()), degree)
    for fam in (orc.BERNOULLI, orc.NORMAL):
        case = ec.deep_chain(fam)
        tabs = case["tabs"]
        assert len(tabs["feat"]) == 49 and tabs["depth"].max() == 24
        paths = orc.route(tabs, 1, case["xc"], None)
        assert (paths[0, :, 24] == 48).sum() == case["claims"]["deepest"] >= 5 and len(set(orc.stops(paths)[0])) >= 20
    case = ec.many_trees()
    assert len(case["tabs"]["tree_off"]) == 1025 and len(case["y"]) == 257
    # the global-scratch rewrite: four leaves, every round of 64 rows holds all four, and the lead lane of a leaf moves
    for fam in (orc.POISSON, orc.NORMAL):
        case = ec.rewrite(fam)
        ni, nr, _ = _mtree.stat_cols(fam)
        assert len(case["tabs"]["feat"]) * (ni + min(nr, 1)) > _mtree.LDS_SLOTS and len(case["tabs"]["feat"]) * 2 > _mtree.LDS_SLOTS
        stops = orc.stops(orc.route(case["tabs"], 2, case["xc"], None))[0]
        leaves = [v for v in set(stops) if case["tabs"]["feat"][v] < 0]
        assert len(leaves) == 4 and (stops == 0).sum() > 100 and ((stops == 1) | (stops == 2)).sum() > 100
        first = [[int(np.flatnonzero(stops[r * 64:(r + 1) * 64] == v)[0]) for v in leaves] for r in range(8)]
        assert all(len(set(col)) >= 3 for col in zip(*first))
    # slabs
    assert _mtree.slabs_for(65537, 7, 2) == 64
    spans = ec.slab_spans(65537, 64)
    assert spans[0] == (0, 1088) and spans[60] == (65280, 65537) and spans[61:] == [(s * 1088, s * 1088) for s in (61, 62, 63)]
    spans = ec.slab_spans(65, 64)
    assert spans[:2] == [(0, 64), (64, 65)] and all(lo == hi for lo, hi in spans[2:])
    assert ec.slab_spans(5000, 1) == [(0, 5000)] and _mtree.slabs_for(5000, 7, 2) == 5 and _mtree.slabs_for(65, 7, 2) == 1


@pytest.mark.parametrize("fam,degree", [(orc.BERNOULLI, 0), (orc.CATEGORICAL, 16), (orc.CATEGORICAL, 3), (orc.POISSON, 0),
                                        (orc.EXPONENTIAL, 0), (orc.NORMAL, 0)])
def test_predict_cases_reach_what_they_name(fam, degree):
    """Rows stop at inner nodes, h_g = 0 and 1 lie on walked paths, a tree has probability 0, the NaN values occur in some
    rows and not in all, and the oracle alone has a clear margin in at least 90 % of the rows of a class test."""
    for n in (1, 255, 256, 257):
        case = ec.predict_case(fam, n, degree)
        tabs, st = case["tabs"], case["state"]
        assert (st["prob"] == 0).sum() == 1 and st["prob"].sum() == 1.0
        paths = orc.route(tabs, 2, case["xc"], None)
        if n < 255:
            continue
        stops = orc.stops(paths)
        assert (tabs["feat"][stops] >= 0).any(axis=1).all()          # in every tree some row stops at an inner node
        walked = np.unique(paths[paths >= 0])
        inner = walked[tabs["feat"][walked] >= 0]
        assert (st["g"][inner] == 0).any() and (st["g"][inner] == 1).any() and ((st["g"][inner] > 0) & (st["g"][inner] < 1)).any()
        a = (tabs, st, fam, degree, 2, case["xc"], None)
        if fam in (orc.BERNOULLI, orc.CATEGORICAL):
            f64, ld = orc.predict(*a, "proba"), orc.predict_ld(*a, "proba")
            bound = 4 * orc.entry_err(f64, ld) + 64 * EPS
            top = np.sort(f64, axis=1)
            assert (top[:, -1] - top[:, -2] > 2 * bound.max(axis=1) * top[:, -1]).mean() >= 0.9
        if fam in (orc.EXPONENTIAL, orc.NORMAL):
            want = orc.predict(*a, "mean" if fam == orc.EXPONENTIAL else "var")
            assert 0 < np.isnan(want).sum() < n
    sym = ec.predict_case(orc.BERNOULLI, 257, symmetric=True)
    proba = orc.predict(sym["tabs"], sym["state"], orc.BERNOULLI, 0, 2, sym["xc"], None, "proba")
    assert np.array_equal(proba[:, 0], proba[:, 1])


def test_one_past_a_limit_is_refused_without_a_gpu():
    from bayesml_amd import _mtree
    from bayesml_amd._engine import EngineLimitError
    for tabs in (ec.chain(25), ec.stumps(1025)):
        with pytest.raises(EngineLimitError, match="bayesml itself has no such limit"):
            _mtree.MtreePass(_mtree.FlatForest(**tabs), orc.BERNOULLI, 0, 1, 0, [], [0.5, 0.5])
    for tabs in (ec.chain(24), ec.stumps(1024)):
        flat = _mtree.FlatForest(**tabs)
        _mtree.check_limits(flat.n_trees, flat.max_tree_nodes, flat.max_children, flat.max_depth)
