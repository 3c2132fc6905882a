"""contexttree without a GPU: the NumPy oracle against the reference's fixtures, the host logic of the drop-in through the
CPU stand-in of the engine, and the argument checks of the ctree_* entry points."""
import ctypes
import json
import os
import pickle
import warnings

import numpy as np
import pytest

import contexttree_oracle as orc
import fake_contexttree_engine as fake
from conftest import GOLDEN, load_golden

NAMES = [c["name"] for c in orc.CASES]


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _cpu_model():
    """A LearnModel subclass whose engine is the stand-in (the seam is a class attribute, so constructors that need the
    tables work too)."""
    ct = _ct()
    return type("CpuLearnModel", (ct.LearnModel,), {"_ctree_pass_factory": staticmethod(fake.CpuCtreePass)})


def test_import_and_export():
    """Fails without the feature: the package does not exist on the parent commit."""
    import bayesml_amd
    ct = _ct()
    assert bayesml_amd.contexttree is ct and "contexttree" in bayesml_amd.__all__
    node = ct._Node(1, 3)
    assert sorted(vars(node)) == ["children", "depth", "h_beta_vec", "h_g", "leaf", "map_leaf", "theta_vec"]
    assert node.children == [None] * 3 and node.h_g == 0.5 and not node.leaf and not node.map_leaf


@pytest.mark.parametrize("name", NAMES)
def test_fixture_inputs_are_the_seeded_recipe(name):
    fx, inp = load_golden(f"contexttree_{name}.npz"), orc.case_inputs(orc.case_by_name(name))
    for key, a in inp.items():
        assert np.array_equal(fx[key], a), key


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference(name):
    """The batch form against the reference's sequential update: beta and the node set exactly, h_g in log-odds to the
    ref_vs_batch that the generator recorded for the case."""
    case = orc.case_by_name(name)
    fx, inp = load_golden(f"contexttree_{name}.npz"), orc.case_inputs(case)
    stages = orc.oracle_stages(_ct(), case, inp)
    assert ("after2" in stages) == (case["n2"] > 0)
    for stage, t in stages.items():
        ex = fx[f"{stage}_exists"]
        assert np.array_equal(t["exists"], ex)
        assert np.array_equal(t["beta"][ex != 0], fx[f"{stage}_beta"][ex != 0])
        assert np.array_equal(t["leaf"][ex != 0], fx[f"{stage}_leaf"][ex != 0])
        assert orc.log_odds_err(t["g"], fx[f"{stage}_g"], ex) <= float(fx["ref_vs_batch"])
    # the MAP sweep on the reference's own posterior
    last = "after2" if case["n2"] else "after1"
    t = {n: fx[f"{last}_{n}"] for n in ("g", "beta", "exists", "leaf")}
    hn_g = case["hn2"][0] if case["hn2"] else case["h0_g"]
    ml = orc.map_tables(case["k"], case["D"], t, hn_g)
    in_tree = fx["map_in_tree"] != 0
    assert np.array_equal(ml[in_tree], fx["map_leaf"][in_tree])


@pytest.mark.parametrize("name", NAMES)
def test_exact_oracle_matches_reference(name):
    """``batch_update_exact`` (mpmath) against the reference's fixtures, to the bound the GPU's posterior is held to:
    4 x ref_vs_batch + 64 eps in log-odds.  Pins the exact oracle of tests/test_gpu_contexttree_rows.py to the reference."""
    case = orc.case_by_name(name)
    fx, inp = load_golden(f"contexttree_{name}.npz"), orc.case_inputs(case)
    stages = orc.exact_stages(_ct(), case, inp)
    assert ("after2" in stages) == (case["n2"] > 0)
    tol = 4 * float(fx["ref_vs_batch"]) + 64 * np.finfo(float).eps
    for stage, t in stages.items():
        ex = fx[f"{stage}_exists"]
        assert np.array_equal(t["exists"], ex)
        assert np.array_equal(t["beta"][ex != 0], fx[f"{stage}_beta"][ex != 0])
        assert orc.log_odds_err(t["g"], fx[f"{stage}_g"], ex) <= tol


def test_exact_logdm_matches_gammaln_on_benign_rows():
    """Small priors and counts, where scipy's gammaln loses nothing: ``logdm`` is within 64 eps row_scale of
    ``logdm_exact``; and two rows worked out by hand."""
    rng, eps = np.random.default_rng(31), np.finfo(float).eps
    for k in (2, 3, 4, 7):
        for _ in range(25):
            b = rng.choice([0.5, 1.0, 1.5, 2.5], k)
            n = rng.integers(0, 40, k)
            if n.sum() == 0:
                continue
            exact, scale = orc.logdm_exact(b, n), orc.row_scale(b, n)
            assert scale >= abs(float(exact))
            assert abs(float(orc.logdm(b, n.astype(float)) - exact)) <= 64 * eps * scale, (b, n)
    # lnDM((1, 1), (1, 0)) = ln(1/2); lnDM((1, 1), (1, 1)) = ln(1 * 1 / (2 * 3)); row_scale of the second: 0 + 0 + ln 6
    assert abs(float(orc.logdm_exact([1.0, 1.0], [1, 0])) + np.log(2.0)) < 4 * eps
    assert abs(float(orc.logdm_exact([1.0, 1.0], [1, 1])) + np.log(6.0)) < 4 * eps
    assert abs(orc.row_scale([1.0, 1.0], [1, 1]) - np.log(6.0)) < 4 * eps
    assert abs(orc.row_scale([1.0, 1.0], [2, 0]) - 2 * np.log(2.0) - np.log(3.0)) < 4 * eps   # ln 2! + ln (3!/1!)


def test_oracle_counts_drop_windows_with_bad_symbols():
    """Covers no product code: it pins ``deepest_counts``, the NumPy reference that the GPU bad-symbol test compares
    ctree_count with, to a case worked out by hand."""
    x = np.array([0, 1, 1, 5, 0, 1, 0, 0, -1, 1, 1, 0])
    bad, c = orc.deepest_counts(x, 2, 2)
    # the windows x[i-2..i] free of bad symbols are i = 2, 6, 7, 11: (key, symbol) = (1, 1), (1, 0), (2, 0), (3, 0)
    assert bad == 2 and np.array_equal(c, [[0, 0], [1, 1], [1, 0], [1, 0]])
    assert np.array_equal(orc.deepest_counts(np.array([0, 1, 1, 0, 1]), 2, 2)[1], orc.level_counts([0, 1, 1, 0, 1], 2, 2)[2])


@pytest.mark.parametrize("name", NAMES)
def test_host_logic_matches_reference(name):
    """Every stage of the case through the drop-in on the CPU stand-in: setters, tree scatter and materialisation,
    calc_pred_dist, estimate_params and the pred_and_update trace."""
    case = orc.case_by_name(name)
    fx, inp = load_golden(f"contexttree_{name}.npz"), orc.case_inputs(case)
    out, _ = orc.drive(_ct(), case, inp, make=_cpu_model())
    tol = float(fx["ref_vs_batch"])
    for stage in orc.STAGES:
        if f"{stage}_exists" not in fx:
            assert f"{stage}_exists" not in out
            continue
        ex = fx[f"{stage}_exists"]
        assert np.array_equal(out[f"{stage}_exists"], ex)
        assert np.array_equal(out[f"{stage}_beta"], fx[f"{stage}_beta"])
        assert np.array_equal(out[f"{stage}_leaf"], fx[f"{stage}_leaf"])
        if stage == "final":
            assert orc.trace_g_ok(out["final_g"], fx["final_g"], ex, tol + 64 * np.finfo(float).eps)
        else:
            assert orc.log_odds_err(out[f"{stage}_g"], fx[f"{stage}_g"], ex) <= tol + 64 * np.finfo(float).eps
    for j in range(3):
        # p is a mixture along one path: |dp| <= sum over the path of |dg| <= (D + 1) tol / 4  (measured: 7.6e-12 relative
        # at k3_d3_long, N = 1e5, where the batch form's h_g are 2.6e-11 from the reference's in log-odds)
        np.testing.assert_allclose(out[f"pred{j}"], fx[f"pred{j}"], rtol=1e-13, atol=(case["D"] + 1) * tol / 4)
        assert out[f"pred{j}_argmax"] == fx[f"pred{j}_argmax"]
        assert np.array_equal(out[f"pred{j}_exists"], fx[f"pred{j}_exists"])
    # the trace from the prior repeats the reference's arithmetic; the one from the posterior inherits the posterior's
    # difference (measured here: up to 4.7e-11 relative at k3_d2, where a node has 1 - h_g = 1.6e-9)
    np.testing.assert_allclose(out["trace0_p"], fx["trace0_p"], rtol=1e-12, atol=0)
    for name in ("g", "beta", "exists", "leaf"):
        np.testing.assert_allclose(out[f"trace0_{name}"], fx[f"trace0_{name}"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["trace_p"], fx["trace_p"], rtol=0,
                               atol=orc.trace_p_atol(tol + 64 * np.finfo(float).eps, case["D"]))
    assert np.array_equal(out["trace_p"].argmax(1), fx["trace_p"].argmax(1))
    assert np.array_equal(out["map_in_tree"], fx["map_in_tree"]) and np.array_equal(out["map_leaf"], fx["map_leaf"])
    assert np.array_equal(np.isnan(out["map_theta"]), np.isnan(fx["map_theta"]))
    np.testing.assert_allclose(np.nan_to_num(out["map_theta"]), np.nan_to_num(fx["map_theta"]), rtol=1e-13, atol=0)
    np.testing.assert_allclose(out["map_g"], fx["map_g"], rtol=1e-9, atol=0)


def test_errors_by_name_and_message():
    want = json.load(open(os.path.join(GOLDEN, "contexttree_errors.json")))
    cases = orc.error_cases(_ct(), make=_cpu_model())
    assert sorted(cases) == sorted(want)
    for name, fn in cases.items():
        assert orc.outcome(fn) == want[name], name


def test_refused_sample_leaves_state_untouched():
    m = _cpu_model()(2, 3)
    m.update_posterior(np.array([0, 1, 1, 0, 1, 0, 0, 1]))
    before = m._eng().get_tables()
    for bad in (np.array([0, 1, 2, 0]), np.array([-1, 0, 1])):
        with pytest.raises(_ct()._contexttree.DataFormatError):
            m.update_posterior(bad)
    after = m._eng().get_tables()
    assert all(np.array_equal(before[n], after[n]) for n in before)


def test_tree_round_trip_and_setters():
    ct, LM = _ct(), _cpu_model()
    gen = ct.GenModel(3, 3, h_g=0.9, seed=1).gen_params()
    m = LM(3, 3, 0.4, np.array([1.0, 2.0, 3.0]), gen.root)
    t1 = orc.tree_to_tables(m.hn_root, 3, 3)
    m2 = LM(3, 3, 0.4, np.array([1.0, 2.0, 3.0]))
    m2.set_hn_params(hn_root=m.hn_root)           # materialise -> scatter -> materialise
    t2 = orc.tree_to_tables(m2.hn_root, 3, 3)
    assert all(np.array_equal(t1[n], t2[n]) for n in t1)
    assert t1["exists"].sum() > 4 and t1["leaf"].sum() > 0
    # hn_g / hn_beta_vec reach every existing node; g stays 0 at the maximal depth
    m2.set_hn_params(hn_g=0.25, hn_beta_vec=np.array([2.0, 2.0, 5.0]))
    t3 = orc.tree_to_tables(m2.hn_root, 3, 3)
    ex, off = t3["exists"] != 0, orc.offsets(3, 3)
    assert np.all(t3["g"][:off[3]][ex[:off[3]]] == 0.25) and np.all(t3["g"][off[3]:] == 0.0)
    assert np.all(t3["beta"][ex] == np.array([2.0, 2.0, 5.0]))
    # get_* key order is part of the API (positional reload in base)
    assert list(m.get_hn_params()) == ["hn_g", "hn_beta_vec", "hn_root"]
    assert list(m.get_h0_params()) == ["h0_g", "h0_beta_vec", "h0_root"]
    assert m.get_constants() == {"c_k": 3, "c_d_max": 3} and list(m.get_p_params()) == ["p_theta_vec"]
    m.overwrite_h0_params()                       # h0 <- hn, then hn <- h0 again: the two trees agree afterwards
    t4, t5 = orc.tree_to_tables(m.h0_root, 3, 3), orc.tree_to_tables(m.hn_root, 3, 3)
    # (hn has, on top, the all-zero context path that the closing calc_pred_dist of set_hn_params creates)
    e4 = t4["exists"] != 0
    assert all(np.array_equal(t4[n][e4], t5[n][e4]) for n in t4) and np.all(t5["exists"] >= t4["exists"])
    assert LM(2).hn_root is None


def test_pickle_keeps_the_posterior():
    m = _cpu_model()(2, 3)
    m.update_posterior(np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0]))
    before = orc.tree_to_tables(m.hn_root, 2, 3)
    # (the subclass made by type() is not importable: pickle the state the way pickle would)
    m2 = _cpu_model().__new__(_cpu_model())
    m2.__dict__.update(pickle.loads(pickle.dumps(m.__getstate__())))
    assert m2._engine is None
    after = orc.tree_to_tables(m2.hn_root, 2, 3)
    assert all(np.array_equal(before[n], after[n]) for n in before)
    m.update_posterior(np.array([1, 1, 0]))
    m2.update_posterior(np.array([1, 1, 0]))
    assert np.array_equal(orc.tree_to_tables(m.hn_root, 2, 3)["g"], orc.tree_to_tables(m2.hn_root, 2, 3)["g"])


def test_gen_model_round_trip(tmp_path):
    ct = _ct()
    g = ct.GenModel(2, 3, h_g=0.75, seed=2).gen_params()
    x = g.gen_sample(40)
    assert x.shape == (40,) and x.min() >= 0 and x.max() <= 1
    g2 = ct.GenModel(2, 3, root=g.get_params()["root"], seed=2)
    t1, t2 = orc.tree_to_tables(g.root, 2, 3), orc.tree_to_tables(g2.root, 2, 3)
    assert all(np.array_equal(t1[n], t2[n]) for n in t1)
    theta = g.root.theta_vec.copy()
    g.gen_params(tree_fix=True)
    assert np.array_equal(orc.tree_to_tables(g.root, 2, 3)["exists"], t1["exists"])
    g.save_sample(str(tmp_path / "s.npz"), 7)
    assert np.load(tmp_path / "s.npz")["arr_0"].shape == (7,)
    g.save_h_params(str(tmp_path / "h.pkl"))
    assert ct.GenModel(2, 3).load_h_params(str(tmp_path / "h.pkl")).h_g == 0.75
    with pytest.raises(NotImplementedError):
        g.visualize_model()
    assert theta.shape == (2,)


def test_engine_limit_and_no_gpu():
    import torch
    from bayesml_amd import _ctree
    from bayesml_amd._engine import EngineLimitError, EngineUnavailableError
    ct = _ct()
    for k, d in ((2, 24), (257, 1), (4, 12), (16, 6)):
        with pytest.raises(EngineLimitError):
            ct.LearnModel(k, d)
    ct.LearnModel(2, 23), ct.LearnModel(256, 1), ct.LearnModel(4, 11)
    if not torch.cuda.is_available():
        with pytest.raises(EngineUnavailableError):
            ct.LearnModel(2, 2).update_posterior(np.array([0, 1, 1]))
        with pytest.raises(EngineUnavailableError):
            _ctree.CtreePass(2, 2)


def test_sizes_and_argument_errors_without_a_gpu():
    """Pure argument validation: status codes and messages, nothing touches a device."""
    from bayesml_amd import _ctree
    lib = _ctree.load_library()
    EINVAL, EUNSUP = 1, 2
    assert lib.ctree_table_len(2, 3, 0) == 1 and lib.ctree_table_len(2, 3, 3) == 8 and lib.ctree_table_len(2, 3, -1) == 15
    assert lib.ctree_table_len(3, 2, -1) == 13 and lib.ctree_table_len(1, 4, -1) == 5
    for bad in ((0, 3, 0), (2, 0, 0), (2, 3, 4), (2, 3, -2), (2, 24, 0), (257, 1, 0)):
        assert lib.ctree_table_len(*bad) == -1
    assert lib.ctree_work_len(2, 24) == -1 and lib.ctree_work_len(0, 1) == -1
    # scratch: count slabs (LDS path: 1 + bins each; global path: 1 each), one value and k counts per node above D
    assert lib.ctree_work_len(2, 3) == 1024 * (1 + 16) + 15 + 7 * 2
    assert lib.ctree_work_len(2, 12) == 1024 + (2 ** 13 - 1) + (2 ** 12 - 1) * 2
    p = ctypes.c_void_p(4096)       # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p(4097)

    def msg():
        return lib.ctree_last_error().decode()
    assert lib.ctree_count(0, p, 10, 2, 24, p, p, None) == EUNSUP and "not supported" in msg()
    assert lib.ctree_count(0, p, 10, 0, 2, p, p, None) == EINVAL and "k and D" in msg()
    assert lib.ctree_count(3, p, 10, 2, 2, p, p, None) == EINVAL and "dtype" in msg()
    assert lib.ctree_count(0, p, 0, 2, 2, p, p, None) == EINVAL and "n must be >= 1" in msg()
    assert lib.ctree_count(0, None, 5, 2, 2, p, p, None) == EINVAL and "null" in msg()
    assert lib.ctree_count(0, p, 5, 2, 2, None, p, None) == EINVAL and "null" in msg()
    assert lib.ctree_count(1, odd, 5, 2, 2, p, p, None) == EINVAL and "aligned" in msg()
    assert lib.ctree_count(0, p, 5, 2, 2, odd, p, None) == EINVAL and "aligned" in msg()
    assert lib.ctree_sweep(2, 24, p, p, 0, p, p, p, 0.5, p, None, p, None) == EUNSUP
    assert lib.ctree_sweep(2, 0, p, p, 0, p, p, p, 0.5, p, None, p, None) == EINVAL
    assert lib.ctree_sweep(2, 2, p, p, 3, p, p, p, 0.5, p, None, p, None) == EINVAL and "n_head" in msg()
    assert lib.ctree_sweep(2, 2, p, None, 1, p, p, p, 0.5, p, None, p, None) == EINVAL and "null" in msg()
    assert lib.ctree_sweep(2, 2, None, p, 1, p, p, p, 0.5, p, None, p, None) == EINVAL and "null" in msg()
    assert lib.ctree_sweep(2, 2, p, p, 1, p, p, p, 1.5, p, None, p, None) == EINVAL and "hn_g" in msg()
    assert lib.ctree_sweep(2, 2, p, p, 1, p, p, p, float("nan"), p, None, p, None) == EINVAL and "hn_g" in msg()
    assert lib.ctree_sweep(2, 2, p, p, 1, odd, p, p, 0.5, p, None, p, None) == EINVAL and "misaligned" in msg()
    assert lib.ctree_map(2, 24, p, p, 0.5, p, p, None) == EUNSUP
    assert lib.ctree_map(0, 2, p, p, 0.5, p, p, None) == EINVAL
    assert lib.ctree_map(2, 2, p, None, 0.5, p, p, None) == EINVAL and "null" in msg()
    assert lib.ctree_map(2, 2, p, p, -0.1, p, p, None) == EINVAL and "hn_g" in msg()
    assert lib.ctree_map(2, 2, odd, p, 0.5, p, p, None) == EINVAL and "misaligned" in msg()


def test_halves_differ_from_whole():
    """Two half-length updates are not one full update (the second half starts with head samples again)."""
    a, b = load_golden("contexttree_whole.npz"), load_golden("contexttree_halves.npz")
    assert np.array_equal(np.concatenate([b["x1"], b["x2"]]), a["x1"])
    assert not np.array_equal(a["after1_beta"], b["after2_beta"])
