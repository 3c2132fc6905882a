"""metatree's MTMCMC / REMTMCMC on the MI355X: the growth kernels of include/mtgrow.h against the NumPy restatement
(tests/metatree_mcmc_oracle.py) fed with the same addressed draw tables, whole chains through ``LearnModel``, and the fit end
to end.

What must be exact: every decision and everything integer (feat, division flags, the lowest row, the counts, the slot every
row reaches, accept flags, the exchange list) and the thresholds, bit for bit.  Every case asserts first that the oracle's own
comparisons (keep / flip, accept, exchange, the 2-means best against second-best cost) have a relative margin of at least
1e-9, so that no rounding-level difference can decide one of them.

What carries rounding: L, g and the posteriors.  The oracle folds in plain float64 as the scalar learners do, so the bound is
on the two float64 evaluations of the same formula: 64 eps x scale, with scale = sum over the visited nodes of
(n_v + 2) ln(n_v + 2), which bounds the magnitude of the log-gamma and alpha ln beta terms that enter a node's log marginal
likelihood (they cancel, so the result's own size is no measure).  g = exp(t1 - L) moves by at most the error of its
exponent, so it takes the same bound absolutely.  Count-valued posterior entries are exact; a normal node's m and beta are
sums over its n_v rows and take 64 eps x n_v x the entry's size.
"""
import contextlib
import io
import pickle

import numpy as np
import pytest
import torch

import metatree_mcmc_oracle as mc
import metatree_oracle as orc

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
H0 = {orc.BERNOULLI: [0.5, 0.5], orc.NORMAL: [0.0, 1.0, 1.0, 1.0, 0.0]}


def _case(n, C=2, depth=3, dc=2, dk=1, fam=orc.BERNOULLI, threshold="1d_kmeans", dtype=np.float64, seed=0, kind="random"):
    rng = np.random.default_rng(seed)
    xc = np.round(rng.uniform(-1, 1, (n, dc)), 3)
    xk = rng.integers(0, C, (n, dk))
    if kind == "duplicates":              # five distinct values in every continuous feature
        xc = np.array([0.0, 0.1, 0.35, 0.6, 1.0])[rng.integers(0, 5, (n, dc))]
    elif kind == "constant":              # lo == hi in feature 0: every row goes to the last child
        xc[:, 0] = 0.25
    elif kind == "close":                 # rows 1e-9 apart: allclose makes the root a leaf
        xc = 0.5 + 1e-9 * rng.uniform(-1, 1, (n, dc))
        xk[:] = 1
    elif kind == "gap":                   # an empty middle child of an even split
        xc = np.where(rng.random((n, dc)) < 0.5, rng.uniform(0.0, 0.2, (n, dc)), rng.uniform(0.9, 1.0, (n, dc)))
        xc[0], xc[1] = 0.0, 1.0
    elif kind == "missing_class":         # class 1 never appears
        xk[xk == 1] = 0
    xc = xc.astype(dtype)
    left = xc[:, 0] < 0.1 if dc else xk[:, 0] == 0
    if fam == orc.BERNOULLI:
        y = (rng.random(n) < np.where(left, 0.15, 0.85)).astype(np.int64)
    else:
        y = np.where(left, -1.0, 2.0) + 0.3 * rng.standard_normal(n)
    return dict(xc=xc if dc else None, xk=xk if dk else None, y=y, C=C, depth=depth, dc=dc, dk=dk, fam=fam, threshold=threshold)


GROWTH = {f"n{n}": dict(n=n) for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049)}
GROWTH.update(
    duplicates=dict(n=700, kind="duplicates"), constant=dict(n=300, kind="constant"), close=dict(n=50, kind="close", dk=1),
    gap_c3=dict(n=400, C=3, depth=2, kind="gap", threshold="sample_midpoint"),
    missing_class=dict(n=300, C=3, depth=2, kind="missing_class", threshold="sample_midpoint"),
    depth_cap=dict(n=500, depth=1), c4_f32=dict(n=777, C=4, depth=2, threshold="sample_midpoint", dtype=np.float32),
    kmeans_f32=dict(n=1500, dtype=np.float32), midpoint_c2=dict(n=333, threshold="sample_midpoint"),
    normal=dict(n=600, fam=orc.NORMAL, dk=0), one_block=dict(n=900, depth=2), categorical_only=dict(n=200, dc=0, dk=3, depth=2))


def _make(case, B):
    from bayesml_amd import _mtgrow
    h0 = H0[case["fam"]]
    cfg = mc.Config(case["fam"], 0, case["dc"], case["dk"], case["C"], case["depth"], h0, h0, 0.5, 0.5, case["threshold"])
    gr = _mtgrow.Grower(case["fam"], 0, case["dc"], case["dk"], [case["C"]] * case["dk"], case["C"], case["depth"], h0, h0, 0.5,
                        0.5, case["threshold"], B, case["xc"], case["xk"], case["y"], device=torch.device("cuda", 0))
    return cfg, gr


def _scale(want):
    n = want["cnt"][want["cnt"] > 0].astype(float)
    return float(((n + 2) * np.log(n + 2)).sum())


def _check_proposal(cfg, case, got, b, want, with_flags):
    inner_levels = cfg.depth < cfg.max_depth
    assert np.array_equal(got["feat"][b], want["feat"]), "feat"
    cont = (want["feat"] >= 0) & (want["feat"] < cfg.dc)
    assert np.array_equal(got["thr"][b][cont].view(np.int64), want["thr"][cont].view(np.int64)), "thresholds, bit for bit"
    assert np.array_equal(got["node"][b], want["node"]), "row -> slot"
    assert np.array_equal(got["count"][b][inner_levels], want["cnt"][inner_levels]), "counts"
    seen = inner_levels & (want["cnt"] > 0)
    assert np.array_equal(got["first"][b][seen], want["first"][seen]), "lowest row"
    leaf = seen & (want["feat"] < 0)
    assert np.array_equal(got["differs"][b][seen] == 0, leaf[seen]), "the allclose leaf flag"
    if with_flags:
        assert np.array_equal(got["dflag"][b], want["dflag"]), "division flags"
    tol = 64 * EPS * _scale(want)
    print(f"chain {b}: L {got['l_new'][b]!r} vs {want['L']!r}, bound {tol:.3e}; max |dg| {np.abs(got['g'][b] - want['g']).max():.3e}")
    assert abs(got["l_new"][b] - want["L"]) <= tol
    assert np.abs(got["g"][b] - want["g"]).max() <= tol
    visited = want["cnt"] > 0
    if case["fam"] == orc.BERNOULLI:
        assert np.array_equal(got["post"][b][visited], want["post"][visited])
    else:
        assert np.array_equal(got["post"][b][visited][:, [1, 2, 4]], want["post"][visited][:, [1, 2, 4]])
        for col in (0, 3):
            bound = 64 * EPS * want["cnt"][visited] * np.maximum(np.abs(want["post"][visited][:, col]), 1.0)
            assert np.all(np.abs(got["post"][b][visited][:, col] - want["post"][visited][:, col]) <= bound), col
    assert np.array_equal(got["post"][b][~visited], want["post"][~visited]), "a slot no row reaches keeps the prior"


@pytest.mark.parametrize("name", list(GROWTH))
def test_growth_against_oracle(name):
    """Two proposals of two chains: the initial tree (every node regenerated), then one with a kept region under g_max = 0.7,
    every level of both against the oracle."""
    case, B = _case(**GROWTH[name]), 2
    cfg, gr = _make(case, B)
    xc = None if case["xc"] is None else case["xc"].astype(np.float64)
    margins = []
    d0, d1 = mc.node_table(11, 0, B, cfg.cap), mc.node_table(11, 1, B, cfg.cap)
    first = [mc.grow(cfg, xc, case["xk"], case["y"], mc.TableDraws(d0), b, None, 0.0, margins) for b in range(B)]
    second = [mc.grow(cfg, xc, case["xk"], case["y"], mc.TableDraws(d1), b, first[b], 0.7, margins) for b in range(B)]
    assert min(margins, default=1.0) >= 1e-9, "the case itself is too close to call"
    l_last, bad = gr.start(d0)
    assert bad == 0
    got = gr.proposal()
    for b in range(B):
        _check_proposal(cfg, case, got, b, first[b], False)
    gr.grow(d1, False, 0.7)
    gr.score()
    got = gr.proposal()
    for b in range(B):
        _check_proposal(cfg, case, got, b, second[b], True)
    if name == "close":
        assert first[0]["feat"][0] == -1 and got["feat"][0, 0] == -1
    gr.close()


def test_one_level_only():
    """mtgrow_level for level 0 alone: the root's decision, first row, count, thresholds and the row -> child map."""
    case, B = _case(n=1025, depth=3), 3
    cfg, gr = _make(case, B)
    d0 = mc.node_table(5, 0, B, cfg.cap)
    gr.grow(d0, True, 0.0, levels=1)
    got = gr.proposal()
    for b in range(B):
        want = mc.grow(cfg, case["xc"], case["xk"], case["y"], mc.TableDraws(d0), b, None, 0.0, levels=1)
        assert got["feat"][b, 0] == want["feat"][0] and got["first"][b, 0] == 0 and got["count"][b, 0] == 1025
        assert np.array_equal(got["thr"][b, 0].view(np.int64), want["thr"][0].view(np.int64))
        assert np.array_equal(got["node"][b], want["node"])
        assert np.array_equal(got["open"][b, :3], [1, 1, 1]) and not got["open"][b, 3:].any()
    gr.close()


# ---- whole chains through the model, on the fixtures' inputs ----------------------------------------------------------------
def _model(case, device="cuda:0"):
    from bayesml_amd import bernoulli, linearregression, metatree, normal
    sub = dict(bernoulli=bernoulli, normal=normal, linearregression=linearregression)[case["sub"]]
    consts = {"c_degree": case["dc"]} if case["sub"] == "linearregression" else {}
    return metatree.LearnModel(case["dc"], case["dk"], c_max_depth=case["depth"], c_num_children_vec=case["C"], SubModel=sub,
                               sub_constants=consts, device=device)


def _fit(model, case, inp, **kw):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        model.fit(inp["xc"], inp["xk"] if case["dk"] else None, inp["y"], alg_type=case["alg"], threshold_type=case["threshold"],
                  **kw)
    return out.getvalue()


@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_whole_chain_against_oracle(case):
    """The engine through ``LearnModel`` against the restatement in mode (b), both on the addressed tables of one seed."""
    inp, kw, seed = mc.case_inputs(case), dict(case["kw"]), 17
    cfg = mc.case_config(case)
    B = kw.get("num_chains", 1)
    tr, trees, prob = mc.run_case(case, mc.Addressed(seed, B, cfg.cap, kw.get("num_exchange", 4)))
    assert min(tr["margins"]) >= 1e-9, "the case itself is too close to call"
    m = _model(case)
    _fit(m, case, inp, seed=seed, **kw)
    out = np.array(m._mcmc_trace["out"])                       # [steps, B, 4]
    assert np.array_equal(out[:, :, 0].astype(bool), np.array(tr["accept"], dtype=bool).reshape(out.shape[:2])), "accept flags"
    if case["alg"] == "REMTMCMC":
        assert m._mcmc_trace["exchange"] == tr["exchange"], "exchange list"
    else:
        assert np.allclose(m._mcmc_trace["g_max"], tr["g_max"], rtol=64 * EPS, atol=0)
    n = case["n"]
    scale = (n + 2) * np.log(n + 2) * (case["depth"] + 1)      # every level's nodes hold n rows together
    l_err = np.abs(out[:, :, 1] - np.array(tr["l_new"]).reshape(out.shape[:2])).max()
    want = m._forest_from_tables(trees, prob)                  # (the layout only: the oracle's list is merged already)
    got = m._hn_forest()
    g_err = np.abs(got.state["g"] - want.state["g"]).max() if got.state["g"].shape == want.state["g"].shape else np.inf
    print(f"{case['name']}: max |dL| per step {l_err:.3e}, max |dg| {g_err:.3e}, bound {64 * EPS * scale:.3e}; "
          f"accepted {int(out[:, :, 0].sum())} of {out[:, :, 0].size}, {len(trees)} trees")
    assert l_err <= 64 * EPS * scale
    assert want.flat.n_trees == len(trees)
    for k, v in want.flat.arrays().items():
        if k == "thr":
            assert np.array_equal(got.flat.thr.view(np.int64), v.view(np.int64)), "thresholds, bit for bit"
        else:
            assert np.array_equal(getattr(got.flat, k), v), k
    assert np.allclose(got.state["prob"], want.state["prob"], rtol=4 * EPS, atol=0)
    assert g_err <= 64 * EPS * scale
    if case["sub"] == "bernoulli":
        assert np.array_equal(got.state["post"], want.state["post"])
    else:       # sums over at most n rows: 64 eps x n x the column's size
        size = np.abs(want.state["post"]).max(axis=0)
        p_err = (np.abs(got.state["post"] - want.state["post"]) / np.maximum(size, 1e-300)).max()
        print(f"{case['name']}: post {p_err:.3e}, bound {64 * EPS * n:.3e}")
        assert p_err <= 64 * EPS * n
    # two runs give identical bits
    m2 = _model(case)
    _fit(m2, case, inp, seed=seed, **kw)
    again = m2._hn_forest()
    assert np.array_equal(np.array(m2._mcmc_trace["out"]).view(np.int64), out.view(np.int64))
    for k in ("g", "post", "prob", "lcm", "lml"):
        assert np.array_equal(again.state[k].view(np.int64), got.state[k].view(np.int64)), k
    assert np.array_equal(again.flat.thr.view(np.int64), got.flat.thr.view(np.int64))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _planted(n=2000, seed=1):
    """Two planted levels of splits: x1 at the root (< 0 against >= 0), then x0 on the left and x3 on the right; x2 is noise.
    (With one second-level split only, a tree rooted at that split's feature computes the same function, and which of the
    two equivalent trees a finite chain visits most is not a property of the engine.)"""
    rng = np.random.default_rng(seed)
    xc = rng.uniform(-1, 1, (n, 4))
    p = np.where(xc[:, 1] < 0, np.where(xc[:, 0] < 0, 0.03, 0.35), np.where(xc[:, 3] < 0, 0.6, 0.97))
    return xc, (rng.random(n) < p).astype(np.int64)


@pytest.mark.parametrize("alg", ["MTMCMC", "REMTMCMC"])
def test_fit_recovers_a_planted_split(alg):
    from bayesml_amd import metatree
    xc, y = _planted()
    m = metatree.LearnModel(4, 0, c_max_depth=2, device="cuda:0")
    with contextlib.redirect_stdout(io.StringIO()) as out:
        m.fit(xc, None, y, alg_type=alg, seed=2)
    text = out.getvalue()
    assert text.startswith("brun_in: 100\n") and ("burn_in + num_metatrees: 600\n" if alg == "MTMCMC" else "num_metatrees: 500\n") in text
    trees, prob = m.hn_metatree_list, m.hn_metatree_prob_vec
    assert abs(prob.sum() - 1) < 1e-12
    best = trees[int(np.argmax(prob))]
    assert best.k == 1 and abs(best.thresholds[1]) < 0.1, (best.k, best.thresholds)
    xt, yt = _planted(1000, seed=9)
    acc = (m.predict(xt, None) == yt).mean()
    root_only = max(yt.mean(), 1 - yt.mean())
    print(f"{alg}: {len(trees)} trees, accuracy {acc:.3f} against the root-only {root_only:.3f}")
    assert acc > root_only + 0.1
    m2 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m2.predict(xt, None), m.predict(xt, None))


def test_given_mt_after_mcmc_equals_the_oracle():
    """A later 'given_MT' update of the forest MTMCMC left: the exact batch oracle on the installed tables."""
    from bayesml_amd import metatree
    xc, y = _planted(400)
    m = metatree.LearnModel(4, 0, c_max_depth=2, device="cuda:0")
    with contextlib.redirect_stdout(io.StringIO()):
        m.fit(xc, None, y, alg_type="MTMCMC", burn_in=20, num_metatrees=40, seed=3)
    before = m._hn_forest().copy()
    x2, y2 = _planted(150, seed=5)
    m.update_posterior(x2, None, y2, alg_type="given_MT")
    got = m._hn_forest()
    want, _ = orc.batch_update(before.flat.arrays(), before.state, orc.BERNOULLI, 0, np.array([0.5, 0.5]), 4, x2, None, y2)
    assert np.array_equal(got.state["post"], want["post"])
    # per tree at most 7 nodes of at most 550 rows each (both batches): the scale of the module docstring
    tol = 64 * EPS * 7 * 552 * np.log(552)
    seen = ~np.isnan(want["lml"])
    errs = dict(g=np.abs(got.state["g"] - want["g"]).max(), lml=np.abs(got.state["lml"][seen] - want["lml"][seen]).max(),
                ln_prob=np.abs(np.log(got.state["prob"]) - np.log(want["prob"])).max())
    print(errs, "bound", tol)
    assert np.array_equal(np.isnan(got.state["lml"]), ~seen)
    assert errs["g"] <= tol and errs["lml"] <= tol and errs["ln_prob"] <= 2 * tol
