"""metatree on the MI355X: mtree_route / mtree_reduce / mtree_sweep / mtree_predict against the reference's fixtures (replayed
with 'given_MT' from the stored forest, so nothing here needs scikit-learn) and against the exact oracle.

Tolerances.  The fixtures hold the reference's float64 values and, per case, ``ref_vs_batch_*``: the reference's own
deviation from the exact batch form.  The state tables are held to 4 x ref_vs_batch + 64 eps in the metric of that table
(h_g: ``log_odds_err``; ln prob_vec: absolute; post, lml, lcm: relative per array); counts and everything integer-valued
exactly.  Every float read-out (predict / predict_proba, pred_var, pred_density, feature_importances) is held, relative per
array, to 4 x its own ``ref_vs_batch_<read-out>`` + 64 eps: the reference's read-out against the float64 oracle's read-out on
the exact state.  Against the exact oracle (the edge cases of the reduction) there is no reference error to allow for: post to
64 eps, and lml to 64 eps of the largest term that enters it (``_lml_scale``), since the terms cancel.
"""
import pickle

import numpy as np
import pytest
import torch

import metatree_oracle as orc
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NAMES = [c["name"] for c in orc.CASES]
CASE = {c["name"]: c for c in orc.CASES}


def _subs():
    from bayesml_amd import bernoulli, categorical, exponential, normal, poisson
    return dict(bernoulli=bernoulli, categorical=categorical, poisson=poisson, exponential=exponential, normal=normal)


def _mt():
    from bayesml_amd import metatree
    return metatree


def _forest_of(fx):
    return {k: fx[k] for k in orc.STRUCT}, fx["init_g"], fx["init_prob"]


def _tols(fx):
    return {k: 4 * float(fx["ref_vs_batch_" + k]) + 64 * EPS for k in ("g", "post", "lml", "prob")}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_replay(name):
    """Both update stages, prob_vec and every read-out of the fixture case, from its stored forest."""
    fx, case = load_golden(f"metatree_{name}.npz"), CASE[name]
    fam = orc.FAMILY[case["sub"]]
    out = orc.drive(_mt(), _subs(), case, orc.case_inputs(case), forest=_forest_of(fx))
    tol = _tols(fx)
    for k in orc.STRUCT:
        assert np.array_equal(out[k], fx[k]), k
    for stage in ("after1", "after2"):
        errs = orc.state_errs({k: out[f"{stage}_{k}"] for k in orc.STATE}, {k: fx[f"{stage}_{k}"] for k in orc.STATE})
        lcm = orc.rel_err(out[f"{stage}_lcm"], fx[f"{stage}_lcm"])
        print(f"{name} {stage}: {errs}, lcm {lcm:.3e}; bounds {tol}")
        assert errs["g"] <= tol["g"] and errs["post"] <= tol["post"] and errs["lml"] <= tol["lml"] and errs["prob"] <= tol["prob"]
        assert lcm <= tol["lml"]
        assert orc.fixed_points_kept(fx["init_g"], out[f"{stage}_g"])
        post, want = out[f"{stage}_post"], fx[f"{stage}_post"]
        if fam in (orc.BERNOULLI, orc.CATEGORICAL):
            assert np.array_equal(post, want)
        elif fam == orc.POISSON:
            assert np.array_equal(post[:, :2], want[:, :2])
        elif fam == orc.EXPONENTIAL:
            assert np.array_equal(post[:, 0], want[:, 0])
        else:
            assert np.array_equal(post[:, [1, 2, 4]], want[:, [1, 2, 4]])
    read = orc.readout_tols(fx)
    for k in orc.READOUTS:
        if k in fx and np.asarray(fx[k]).dtype.kind == "f":
            err = orc.rel_err(out[k], fx[k])
            print(f"{name} {k}: {err:.3e}, bound {read[k]:.3e}")
            assert err <= read[k], k
    if fam in (orc.BERNOULLI, orc.CATEGORICAL):       # the argmax, wherever the reference's margin is beyond the bound
        top = np.sort(fx["predict_proba"], axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * read["predict_proba"]
        assert clear.mean() > 0.9 and np.array_equal(out["predict"][clear], fx["predict"][clear])
    assert int(out["map_index"]) == int(fx["map_index"]) and np.array_equal(out["map_leaf"], fx["map_leaf"])


# ---- the engine against the exact oracle ----------------------------------------------------------------------------------------
def _binary_tree(depth, n_trees=1):
    """Full binary trees on one continuous feature in [0, 1): leaf j of depth d holds [j, j + 1) / 2^d."""
    from bayesml_amd import _mtree
    feat, child0, nchild, thr_off, dep, thr, tree_off = [], [], [], [], [], [], [0]
    for _ in range(n_trees):
        base = len(feat)
        lo_hi = [(0.0, 1.0)]
        for v in range(2 ** (depth + 1) - 1):
            d = int(np.log2(v + 1))
            lo, hi = lo_hi[v]
            dep.append(d)
            if d == depth:
                feat.append(-1), child0.append(0), nchild.append(0), thr_off.append(-1)
                continue
            mid = (lo + hi) / 2
            feat.append(0), child0.append(base + 2 * v + 1), nchild.append(2), thr_off.append(len(thr))
            thr.extend([lo, mid, hi])
            lo_hi.extend([(lo, mid), (mid, hi)])
        tree_off.append(len(feat))
    i32 = lambda a: np.array(a, np.int32)       # noqa: E731
    return _mtree.FlatForest(i32(tree_off), i32(feat), i32(child0), i32(nchild), i32(thr_off), i32(dep), np.array(thr))


H0 = {orc.BERNOULLI: [0.5, 0.5], orc.CATEGORICAL: [0.5, 0.5, 0.5], orc.POISSON: [1.0, 1.0, 0.0], orc.EXPONENTIAL: [1.0, 1.0],
      orc.NORMAL: [0.0, 1.0, 1.0, 1.0, 0.0]}
DEGREE = {orc.CATEGORICAL: 3}


def _engine(flat, fam, g0=0.5):
    from bayesml_amd import _mtree
    eng = _mtree.MtreePass(flat, fam, DEGREE.get(fam, 0), 1, 0, [], H0[fam], torch.device("cuda", 0))
    st = dict(g=np.where(flat.feat < 0, 0.0, g0), post=np.tile(H0[fam], (flat.n_nodes, 1)), lml=np.full(flat.n_nodes, np.nan),
              lcm=np.zeros(flat.n_nodes), prob=np.ones(flat.n_trees) / flat.n_trees)
    eng.set_state(st)
    return eng, st


def _sample(fam, x, rng):
    if fam == orc.BERNOULLI:
        return (rng.random(len(x)) < x).astype(np.int64)
    if fam == orc.CATEGORICAL:
        return (np.floor(x * 8).astype(np.int64) + rng.integers(0, 2, len(x))) % 3
    if fam == orc.POISSON:
        return rng.poisson(1 + 5 * x)
    if fam == orc.EXPONENTIAL:
        return rng.exponential(0.5 + x)
    return 1e6 + np.floor(x * 8) + 0.01 * rng.standard_normal(len(x))       # a per-leaf offset on a large level


def _lml_scale(fam, post):
    """The largest term of the family's log marginal likelihood over the nodes."""
    from scipy.special import gammaln
    a = np.abs(post)
    if fam in (orc.BERNOULLI, orc.CATEGORICAL):
        return float(np.max(gammaln(a.sum(1) + 1)))
    if fam == orc.NORMAL:
        return float(np.max(np.abs(post[:, 2] * np.log(post[:, 3])) + gammaln(post[:, 2]) + post[:, 4]))
    return float(np.max(np.abs(post[:, 0] * np.log(post[:, 1])) + gammaln(post[:, 0] + 1) + (a[:, 2] if post.shape[1] > 2 else 0)))


def _against_oracle(flat, fam, x, y, what):
    eng, st = _engine(flat, fam)
    xc, _ = eng.adopt_x(x[:, None], None)
    n, bad = eng.update(xc, None, eng.adopt_y(y))
    assert (n, bad) == (len(x), 0)
    got = eng.get_state()
    args = (flat.arrays(), st, fam, DEGREE.get(fam, 0), H0[fam], 1, x[:, None], None, y)
    want, counts = orc.batch_update(*args)
    si, _ = eng.last_stats()
    assert np.array_equal(si[:, 0], counts), what
    # per node and per column: integer-valued columns exactly, real ones against the reference's own per-node float64 form
    scales = orc.m_scales(flat.arrays(), st, 1, x[:, None], None, y) if fam == orc.NORMAL else None
    node, bound = orc.node_errs(fam, got["post"], want["post"], scales), orc.post_bounds(fam, orc.plain_update(*args)["post"],
                                                                                         want["post"], scales)
    for c in range(node.shape[1]):
        print(f"{what}: post[:, {c}] {node[:, c].max():.3e}, bound {bound.get(c, 0.0):.3e}")
        assert node[:, c].max() <= bound.get(c, 0.0), (what, c)
    errs = orc.state_errs(got, want)
    seen = ~np.isnan(want["lml"])
    scale = _lml_scale(fam, want["post"][seen])
    lml_err = float(np.max(np.abs(got["lml"][seen] - want["lml"][seen]))) / scale
    print(f"{what}: {errs}; lml {lml_err:.3e} of its largest term")
    assert np.array_equal(np.isnan(got["lml"]), ~seen)
    assert errs["post"] <= 64 * EPS and lml_err <= 64 * EPS and errs["prob"] <= 64 * EPS * max(1.0, scale), what
    # log-odds are differences of L values of the size of `scale`
    assert errs["g"] <= 64 * EPS * max(1.0, scale), what
    untouched = ~seen
    assert np.array_equal(got["post"][untouched], st["post"][untouched]) and np.array_equal(got["g"][untouched], st["g"][untouched])
    return eng


@pytest.mark.parametrize("fam", [orc.BERNOULLI, orc.CATEGORICAL, orc.POISSON, orc.EXPONENTIAL, orc.NORMAL])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_reduction_edges(fam, n):
    """Wave and slab edges of the reduction: N = 63, 64, 65, and one slab of 1024 rows plus one row."""
    rng = np.random.default_rng(n * 10 + fam)
    x = rng.random(n)
    _against_oracle(_binary_tree(3, 2), fam, x, _sample(fam, x, rng), f"family {fam}, n = {n}")


@pytest.mark.parametrize("fam", [orc.POISSON, orc.NORMAL])
def test_one_leaf_and_64_leaves(fam):
    """64 rows that share a leaf (one group of 64 lanes) and 64 rows on 64 different leaves of a depth-6 tree (64 groups)."""
    rng = np.random.default_rng(6 + fam)
    flat = _binary_tree(6)
    same = np.full(64, 0.3) + rng.random(64) / 1024
    _against_oracle(flat, fam, same, _sample(fam, same, rng), f"family {fam}, one leaf")
    spread = (rng.permutation(64) + 0.5) / 64
    _against_oracle(flat, fam, spread, _sample(fam, spread, rng), f"family {fam}, 64 leaves")


@pytest.mark.parametrize("fam", [orc.BERNOULLI, orc.NORMAL])
@pytest.mark.parametrize("depth", [10, 11])
def test_lds_and_global_tables(fam, depth):
    """Both sides of MTREE_LDS_SLOTS: a depth-10 tree's table (2047 nodes x 2 columns) lives in LDS, a depth-11 tree's
    (4095 x 2) in the wave's slab of global scratch."""
    from bayesml_amd import _mtree
    flat = _binary_tree(depth)
    assert (flat.n_nodes * 2 <= _mtree.LDS_SLOTS) == (depth == 10)
    rng = np.random.default_rng(depth * 10 + fam)
    x = rng.random(300)
    _against_oracle(flat, fam, x, _sample(fam, x, rng), f"family {fam}, depth {depth}")


def test_same_update_twice_is_bitwise_equal():
    """No floating-point atomics: the same update from the same state gives the same bits, real columns included."""
    rng = np.random.default_rng(3)
    flat = _binary_tree(5, 3)
    x = rng.random(5000)
    for fam in (orc.POISSON, orc.EXPONENTIAL, orc.NORMAL):
        y = _sample(fam, x, rng)
        runs = []
        for _ in range(2):
            eng, _ = _engine(flat, fam)
            xc, _ = eng.adopt_x(x[:, None], None)
            eng.update(xc, None, eng.adopt_y(y))
            runs.append((eng.get_state(), eng.last_stats()))
        for k in orc.STATE:
            assert np.array_equal(runs[0][0][k], runs[1][0][k], equal_nan=True), (fam, k)
        assert np.array_equal(runs[0][1][1], runs[1][1][1]), fam


def _hand_model(sub_name, device="cuda:0"):
    mt, subs = _mt(), _subs()
    flat, g = orc._hand_forest()
    m = mt.LearnModel(SubModel=subs[sub_name], device=device, **orc._HAND)
    m.set_hn_params(hn_metatree_list=orc.nodes_from_flat(mt, flat, g, subs[sub_name].LearnModel),
                    hn_metatree_prob_vec=np.array([0.4, 0.6]))
    return m


def test_sample_dtypes_agree_bitwise():
    """u8 / i32 / i64 categoricals and f32 / f64 continuous features are read where they lie and route alike."""
    inp = orc.case_inputs(CASE["threeway"])
    xc32 = inp["xc1"].astype(np.float32)
    ref = None
    for xc, kdt in ((xc32.astype(np.float64), np.int64), (xc32, np.int64), (xc32, np.int32), (xc32, np.uint8)):
        m = _hand_model("bernoulli")
        m.update_posterior(xc, inp["xk1"].astype(kdt), inp["y1"], alg_type="given_MT")
        st = m._hn_forest().state
        if ref is None:
            ref = st
        for k in orc.STATE:
            assert np.array_equal(st[k], ref[k], equal_nan=True), (k, kdt)


def test_bad_categorical_leaves_state_untouched():
    from bayesml_amd import DataFormatError
    inp = orc.case_inputs(CASE["threeway"])
    m = _hand_model("bernoulli")
    m.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    before = {k: np.array(v) for k, v in m._hn_forest().state.items()}
    bad = torch.from_numpy(inp["xk2"].copy())
    bad[7, 0] = 3
    with pytest.raises(DataFormatError):
        m.update_posterior(torch.from_numpy(inp["xc2"]), bad, torch.from_numpy(inp["y2"]), alg_type="given_MT")
    after = m._hn_forest().state
    for k in orc.STATE:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


def test_nan_row_stops_at_its_node():
    """A NaN matches no child: the row counts at every node down to that one and at none below (oracle: the same walk)."""
    rng = np.random.default_rng(11)
    flat = _binary_tree(3)
    x = rng.random(200)
    x[::9] = np.nan
    eng = _against_oracle(flat, orc.POISSON, x, rng.poisson(3.0, 200), "NaN rows")
    si, _ = eng.last_stats()
    assert si[0, 0] == 200 and si[1, 0] + si[2, 0] == 200 - np.isnan(x).sum()


def test_pred_and_update_predicts_then_updates():
    """pred_and_update = the prediction from the state before, then a 'given_MT' update on the same rows."""
    inp = orc.case_inputs(CASE["threeway"])
    a, b = _hand_model("bernoulli"), _hand_model("bernoulli")
    a.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    b.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    want = b.predict_proba(inp["xc2"], inp["xk2"])
    b.update_posterior(inp["xc2"], inp["xk2"], inp["y2"], alg_type="given_MT")
    assert np.array_equal(a.pred_and_update(inp["xc2"], inp["xk2"], inp["y2"], loss="KL"), want)
    for k in orc.STATE:
        assert np.array_equal(a._hn_forest().state[k], b._hn_forest().state[k], equal_nan=True), k


def test_predict_refuses_bad_categorical_values():
    from bayesml_amd import DataFormatError
    inp = orc.case_inputs(CASE["threeway"])
    m = _hand_model("bernoulli")
    bad = torch.from_numpy(inp["xkp"].copy()).cuda()
    bad[2, 0] = 3
    with pytest.raises(DataFormatError):
        m.predict(torch.from_numpy(inp["xcp"]).cuda(), bad)


def test_pickle_round_trip():
    inp = orc.case_inputs(CASE["threeway"])
    m = _hand_model("bernoulli")
    m.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    m2 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m.predict_proba(inp["xcp"], inp["xkp"]), m2.predict_proba(inp["xcp"], inp["xkp"]))
