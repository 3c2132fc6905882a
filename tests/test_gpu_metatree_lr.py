"""``metatree`` with SubModel=linearregression on the MI355X: the ordering, the segmented f64-MFMA Gram pass, the sweep and
the predictive fold of include/mtree.h against the exact oracle of tests/metatree_lr_oracle.py, at the smallest shapes at
which each can go wrong (tests/metatree_lr_cases.py).

Bounds (DESIGN.md section 4i's rule, 4 x e_plain + 64 eps, max over nodes, per column group; e_plain is the deviation of
the reference's own per-node float64 formulas, ``lro.plain_update``, from the exact state on the same case):
  n and alpha bit-equal; Lambda_ij relative to |Lambda0_ij| + sum |x_i x_j|; beta relative to
  S_beta = beta0 + (y'y + mu0'Lambda0 mu0 + mu'Lambda mu) / 2; mu as ||d mu||_inf / ||mu||_inf with D cond_2(Lambda) eps
  added, the forward bound of a backward-stable solve.
  lml against the exact formula on the device's OWN post of that node, relative to max(1, |lml|), with the float64
  formula's deviation on the same post as e_plain; g (log-odds), lcm and ln prob against the exact mixture of the device's
  own lml, in units of the largest |lml| of the case (the inputs of the mixture are binary64 numbers of that size, so an
  ulp of them is what a sum of them can carry), within 64 eps.
  Read-outs against the float64 oracle on the device's own state: the mean within 64 eps of sum_j |x_j mu_j| (at most
  D + depth + trees < 32 roundings on either side); variance and density relative within (64 + 4 D cond_2(Lambda)) eps
  (x'Lambda^-1 x through the inverse factor on one side and a solve on the other: twice the forward bound each).
Every test prints its measured figures beside the bounds.
"""
import numpy as np
import pytest
import torch

import metatree_lr_cases as lc
import metatree_lr_oracle as lro
import metatree_oracle as orc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _engine(case, state=None):
    from bayesml_amd import _mtree
    eng = _mtree.MtreePass(_mtree.FlatForest(**case["tabs"]), _mtree.LINREG, case["D"], case["dim_cont"], case["dim_cat"],
                           case["cat_card"], case["h0"], torch.device("cuda", 0))
    eng.set_state(case["state"] if state is None else state)
    return eng


def _update(eng, case):
    xc, xk = eng.adopt_x(case["xc"], case["xk"])
    n, bad = eng.update(xc, xk, eng.adopt_y(case["y"]))
    assert (n, bad) == (len(case["y"]), 0), case["name"]
    return eng.get_state()


def _judge(case, got, state=None, eng=None):
    """``got`` against the exact update of ``state`` in the metrics of the module docstring.  Returns the exact state."""
    before = case["state"] if state is None else state
    D, name = case["D"], case["name"]
    xc64 = np.asarray(case["xc"], dtype=np.float64)
    args = (case["tabs"], before, D, case["h0"], case["dim_cont"], xc64, case["xk"], case["y"])
    want, counts, info = lro.batch_update(*args)
    plain = lro.plain_update(*args)
    visited = counts > 0
    if eng is not None:
        assert np.array_equal(eng.last_stats()[0][:, 0], counts), name
    e_got = lro.post_errs(got["post"], want["post"], D, info, visited)
    e_plain = lro.post_errs(plain["post"], want["post"], D, info, visited)
    bounds = lro.post_bounds(e_plain, D, e_got["cond"])
    for k in ("lam", "beta", "mu"):
        print(f"{name}: {k} err {e_got[k]:.3e} ({e_got[k] / EPS:.1f} eps) bound {bounds[k]:.3e} e_plain {e_plain[k]:.3e} "
              f"cond {e_got['cond']:.3e}")
    assert e_got["n"] == 0 and e_got["alpha"] == 0, (name, "n and alpha must be bit-equal")
    for k in ("lam", "beta", "mu"):
        assert e_got[k] <= bounds[k], (name, k, e_got[k], bounds[k])
    assert lro.unchanged_where_unvisited(before, got, visited), name
    assert np.array_equal(np.isnan(got["lml"]), np.isnan(want["lml"])), name
    d = lro.decomposed_errs(case["tabs"], before, got, D, case["h0"], visited)
    lml_bound = 4 * d["lml_plain"] + 64 * EPS
    print(f"{name}: lml err {d['lml']:.3e} bound {lml_bound:.3e}; g {d['g']:.3e} lcm {d['lcm']:.3e} prob {d['prob']:.3e} "
          f"bound {64 * EPS * d['scale']:.3e} (scale {d['scale']:.3e})")
    assert d["lml"] <= lml_bound, (name, "lml", d["lml"], lml_bound)
    for k in ("g", "lcm", "prob"):
        assert d[k] <= 64 * EPS * d["scale"], (name, k, d[k])
    assert orc.fixed_points_kept(before["g"], got["g"]), name
    return want


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_quad_padding(n):
    case = lc.quad_padding(n)
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("D", [2, 14, 15])
def test_tile_edge(D, dtype):
    case = lc.tile_edge(D, dtype)
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


def test_row_stride_at_the_c_abi():
    """x read through a row stride larger than D gives the same bits as the packed matrix."""
    case = lc.tile_edge(14, np.float64)
    eng = _engine(case)
    xc, xk = eng.adopt_x(case["xc"], None)
    y = eng.adopt_y(case["y"])
    stop, _, _ = eng.route(xc, xk)
    eng.reduce_x(stop, xc, y)
    packed = [t.clone() for t in (eng.stat_int, eng.stat_real)]
    wide = torch.full((xc.shape[0], 19), float("nan"), dtype=xc.dtype, device=xc.device)
    wide[:, :14] = xc
    view = wide[:, :14]
    assert view.stride(0) == 19
    eng.stat_real.fill_(-1.0)
    eng.reduce_x(stop, view, y)
    assert torch.equal(eng.stat_int, packed[0]) and torch.equal(eng.stat_real, packed[1])


@pytest.mark.parametrize("kind", ["crossing", "ending", "three_blocks"])
def test_block_edges(kind):
    from bayesml_amd import _mtree
    case, (left, right) = lc.block_edge(kind, _mtree.LR_BLOCK)
    eng = _engine(case)
    got = _update(eng, case)
    assert list(eng.last_stats()[0][:, 0]) == [left + right, left, right]
    _judge(case, got, eng=eng)


def test_rows_scattered_through_the_batch():
    from bayesml_amd import _mtree
    case = lc.scattered(_mtree.LR_BLOCK)
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


def test_many_tiny_runs_and_empty_leaves():
    case = lc.tiny_runs()
    eng = _engine(case)
    got = _update(eng, case)
    counts = eng.last_stats()[0][:, 0]
    leaves = case["tabs"]["feat"] < 0
    assert (counts[leaves] == 0).any() and (counts[leaves] > 0).sum() >= 8
    assert np.isnan(got["lml"][counts == 0]).all()
    _judge(case, got, eng=eng)


def test_mixed_routing():
    case = lc.mixed_routing()
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


def test_two_stage_update():
    """A second update folds onto the first one's posterior; n in lml is cumulative."""
    case = lc.mixed_routing()
    eng = _engine(case)
    first = _update(eng, case)
    _judge(case, first, eng=eng)
    second = lc.second_stage(case)
    got = _update(eng, second)
    _judge(second, got, state=first, eng=eng)
    D = case["D"]
    assert got["post"][0, D + lro.tri(D) + 2] == len(case["y"]) + len(second["y"])


def test_several_trees():
    case = lc.several_trees()
    eng = _engine(case)
    got = _update(eng, case)
    _judge(case, got, eng=eng)
    assert len(set(got["prob"])) == 3 and abs(got["prob"].sum() - 1.0) < 4 * EPS


def test_precision_edge():
    case = lc.precision_edge()
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


def test_rows_stopping_at_inner_nodes():
    """Engine level, a hand-written stop table: a node's statistics are its own rows' plus its children's totals; a row
    whose stop node is outside its tree is left out."""
    case = lc.several_trees()
    D, n = case["D"], 40
    T = lro.tri(D)
    x, y = case["xc"][:n].copy(), case["y"][:n].copy()
    off = case["tabs"]["tree_off"]
    stop = np.zeros((3, n), dtype=np.int32)
    stop[0] = 0                                                  # root-only tree
    stop[1] = off[1] + np.arange(n) % 3                          # stump: root, left, right in turn
    stop[2] = off[2] + np.arange(n) % 7                          # depth 2: every node in turn
    stop[2, 5], stop[2, 6] = -1, off[1]                          # outside the tree: left out
    eng = _engine(case)
    xc, _ = eng.adopt_x(x, None)
    eng.reduce_x(torch.from_numpy(stop).to(eng.device), xc, eng.adopt_y(y))
    eng.sweep()
    si, sr = eng.last_stats()
    tabs = case["tabs"]
    own = [np.flatnonzero(stop[b] == v) for b in range(3) for v in range(off[b], off[b + 1])]
    below = list(own)
    for v in range(len(own) - 1, -1, -1):
        if tabs["feat"][v] >= 0:
            kids = range(tabs["child0"][v], tabs["child0"][v] + tabs["nchild"][v])
            below[v] = np.concatenate([own[v]] + [below[c] for c in kids])
    iu = np.triu_indices(D)
    for v, rows in enumerate(below):
        assert si[v, 0] == len(rows), v
        want = np.concatenate([(x[rows].T @ x[rows])[iu], x[rows].T @ y[rows], [y[rows] @ y[rows]]])
        scale = np.concatenate([(np.abs(x[rows]).T @ np.abs(x[rows]))[iu], np.abs(x[rows]).T @ np.abs(y[rows]),
                                [y[rows] @ y[rows]]])
        assert sr.shape[1] == T + D + 1
        # at most n + 1 roundings on either side of a sum of n products
        assert np.all(np.abs(sr[v] - want) <= 2 * (n + 1) * EPS * scale), (v, sr[v], want)
    assert si[off[2], 0] == n - 2


def test_two_runs_give_the_same_bits():
    from bayesml_amd import _mtree
    case = lc.scattered(_mtree.LR_BLOCK)
    tables = []
    for _ in range(2):
        eng = _engine(case)
        _update(eng, case)
        tables.append([t.clone() for t in (eng.post, eng.g, eng.lml, eng.lcm, eng.prob, eng.stat_int, eng.stat_real)])
    for a, b in zip(*tables):
        assert torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b))
                                     and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


# ---- read-outs, through the model ---------------------------------------------------------------------------------------------
def _model(case, **sub_h0):
    from bayesml_amd import linearregression, metatree
    D = case["D"]
    consts = dict(c_dim_continuous=D, c_dim_categorical=case["dim_cat"], c_max_depth=4)
    if case["dim_cat"]:
        consts.update(c_num_children_vec=np.array([3, 2, 3]), c_num_assignment_vec=np.array([1, -1, -1]))
    m = metatree.LearnModel(SubModel=linearregression, sub_constants={"c_degree": D}, sub_h0_params=sub_h0, **consts)
    roots = orc.nodes_from_flat(metatree, case["tabs"], case["state"]["g"], lambda: linearregression.LearnModel(D, **sub_h0))
    m.set_hn_params(hn_metatree_list=roots, hn_metatree_prob_vec=np.array(case["state"]["prob"]))
    return m


def _cond(state, D):
    return max(float(np.linalg.cond(lro.unpack(p, D)[1])) for p in state["post"])


def test_readouts_against_the_oracle_on_the_device_s_state():
    case = lc.mixed_routing()
    D = case["D"]
    m = _model(case)
    m.update_posterior(case["xc"], case["xk"], case["y"], alg_type="given_MT")
    st = m._eng().get_state()
    rng = np.random.default_rng(19)
    xp, kp = rng.uniform(-3, 3, size=(257, D)), rng.integers(0, 3, size=(257, 1))
    yp = xp @ np.linspace(1.0, -1.0, D) + rng.standard_normal(257)
    args = (case["tabs"], st, D, D, xp, kp)
    mean = m.predict(xp, kp)
    scale = np.max(np.abs(xp) @ np.abs(st["post"][:, :D]).T, axis=1)
    err = np.max(np.abs(mean - lro.predict(*args, "mean")) / scale)
    print(f"readouts: mean err {err:.3e} of sum |x mu|, bound {64 * EPS:.3e}")
    assert err <= 64 * EPS
    tol = (64 + 4 * D * _cond(st, D)) * EPS
    var = m.calc_pred_dist(xp, kp).calc_pred_var()
    e_var = float(orc.entry_err(var, lro.predict(*args, "var")).max())
    dens = m.calc_pred_density(yp)
    e_den = float(orc.entry_err(dens, lro.pred_density(*args, yp)).max())
    print(f"readouts: var err {e_var:.3e} density err {e_den:.3e} bound {tol:.3e}")
    assert e_var <= tol and e_den <= tol and np.all(var > 0)
    fi = m.calc_feature_importances()
    want = lro.feature_importances(case["tabs"], st, D + 1)
    assert np.all(np.abs(fi - want) <= 64 * EPS * np.nanmax(np.abs(st["lml"])))
    assert np.array_equal(m.make_prediction("squared"), mean)


def test_variance_is_nan_where_nu_is_two():
    """h0_alpha = 0.5: a leaf with one row has nu = 2 and no variance; the NaNs sit where the oracle's do."""
    rng = np.random.default_rng(20)
    x, y = lc.sample(4, 2, seed=21, x0=np.array([-1.0, -0.5, -1.5, 1.0]))
    case = lc.case("nu_two", [lc.STUMP], x, y, h0=lro.pack(np.zeros(2), np.eye(2), 0.5, 1.0))
    m = _model(case, h0_alpha=0.5)
    m.update_posterior(x, None, y, alg_type="given_MT")
    st = m._eng().get_state()
    xp = rng.uniform(-2, 2, size=(33, 2))
    var = m.calc_pred_dist(xp, None).calc_pred_var()
    want = lro.predict(case["tabs"], st, 2, 2, xp, None, "var")
    assert np.array_equal(np.isnan(var), np.isnan(want)) and 0 < np.isnan(var).sum() < len(var)
    assert np.array_equal(np.isnan(var), xp[:, 0] >= 0)
    assert float(orc.entry_err(var, want).max()) <= (64 + 4 * 2 * _cond(st, 2)) * EPS


def test_pred_and_update():
    case = lc.several_trees()
    m = _model(case)
    x, y = case["xc"], case["y"]
    m.update_posterior(x[:300], None, y[:300], alg_type="given_MT")
    before = m.predict(x[300:], None)
    got = m.pred_and_update(x[300:], None, y[300:])
    assert np.array_equal(got, before)
    root = m.hn_metatree_list[0]
    assert root.sub_model._n == 400 and root.sub_model.hn_lambda_mat.shape == (3, 3)
    assert np.array_equal(root.sub_model.hn_lambda_mat, root.sub_model.hn_lambda_mat.T)
    assert not np.array_equal(m.predict(x[300:], None), before)


def test_fit_with_mtrf_on_the_device():
    """MTRF grows the forest with scikit-learn on the host and updates it on the device."""
    pytest.importorskip("sklearn")
    from bayesml_amd import linearregression, metatree
    x, y = lc.sample(600, 3, seed=22)
    y = y + 2.0 * (x[:, 0] > 0)
    m = metatree.LearnModel(3, 0, c_max_depth=3, SubModel=linearregression, sub_constants={"c_degree": 3})
    m.fit(x, None, y, n_estimators=4, random_state=0)
    assert m._engine.launch_info == "mtree_route + mtree_reduce_x + mtree_sweep"
    resid = y - m.predict(x, None)
    assert np.sqrt(np.mean(resid ** 2)) < 1.3 and abs(m.hn_metatree_prob_vec.sum() - 1.0) < 1e-12
    assert all(t.sub_model._n == 600 for t in m.hn_metatree_list)


# ---- the reference's fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in lro.CASES])
def test_fixture_on_the_device(name):
    """The fixture's forest replayed with 'given_MT' through the model, both stages.  post per column group against the
    fixture's exact state within 4 x e_plain + 64 eps (mu: + D cond eps), e_plain recorded by the generator; lml relative,
    g in log-odds and ln prob absolutely against the exact state, and the read-outs relative per array against the
    reference's, each within 4 x ref_vs_batch + 64 eps."""
    from conftest import load_golden
    from bayesml_amd import linearregression, metatree
    fx = load_golden(f"metatree_lr_{name}.npz")
    case = next(c for c in lro.CASES if c["name"] == name)
    D, flat = case["D"], {k: fx[k] for k in orc.STRUCT}
    inp = {k: fx[k].astype(np.int64) if k.startswith("xk") else fx[k] for k in fx if k[:2] in ("xc", "xk") or k[0] == "y"}
    out = lro.drive(metatree, linearregression, case, inp, forest=(flat, fx["init_g"], fx["init_prob"]))
    for tag in ("1", "2"):
        got = {k: out[f"after{tag}_{k}"] for k in orc.STATE}
        exact = {k: fx[f"exact{tag}_{k}"] for k in orc.STATE}
        info = dict(s_beta=fx[f"exact{tag}_s_beta"], lam_scale=fx[f"exact{tag}_lam_scale"])
        e_plain = dict(zip(("lam", "beta", "mu", "cond"), fx[f"e_plain{tag}"]))
        errs = lro.post_errs(got["post"], exact["post"], D, info, fx[f"exact{tag}_counts"] > 0)
        bounds = lro.post_bounds(e_plain, D, errs["cond"])
        assert errs["n"] == 0 and errs["alpha"] == 0, name
        for k in ("lam", "beta", "mu"):
            print(f"{name} stage {tag}: {k} err {errs[k]:.3e} ({errs[k] / EPS:.1f} eps) bound {bounds[k]:.3e}")
            assert errs[k] <= bounds[k], (name, tag, k, errs[k], bounds[k])
        assert np.array_equal(np.isnan(got["lml"]), np.isnan(exact["lml"])), name
        for k, e in lro.state_errs(got, exact).items():
            tol = 4 * float(fx["ref_vs_batch_" + k]) + 64 * EPS
            print(f"{name} stage {tag}: {k} err {e:.3e} bound {tol:.3e}")
            assert e <= tol, (name, tag, k, e, tol)
        assert orc.rel_err(got["lcm"], exact["lcm"]) <= 4 * float(fx["ref_vs_batch_lml"]) + 64 * EPS
    for k in lro.READOUTS:
        if k in out:
            e, tol = orc.rel_err(out[k], fx[k]), 4 * float(fx["ref_vs_batch_" + k]) + 64 * EPS
            print(f"{name}: {k} err {e:.3e} bound {tol:.3e}")
            assert e <= tol, (name, k, e, tol)
