"""The meta-tree engine (``_mtree.MtreePass``) on the MI355X against the exact oracle at the edges of every branch: the
conditioning of the real columns, the fixed points and the far ends of the mixture, the limits of the tables, the switch
between the LDS and the global-scratch table, the slab arithmetic, and the predictive fold on hand-set states.  The cases
come from tests/metatree_edge_cases.py; tests/test_metatree.py checks without a GPU that each reaches the branch it names.

Bounds.  ``post`` is judged per node and per column (``orc.node_errs``): integer-valued columns bit-equal to the exact
state; a real column within 4 x e_plain + 64 eps, e_plain the deviation of the reference's own per-node float64 formulas
(``orc.plain_update``) from the exact state on the same case, max over nodes.  h_g in log-odds, lml, lcm and ln prob to
64 eps of the largest term of the case's log marginal likelihoods, as in test_gpu_metatree.py.  Predictions to
4 x e64 + 64 eps relative per entry, e64 the float64 oracle's own deviation from the long-double fold, NaN patterns equal.
Every test prints its measured deviation beside its bound; profiles/mtree.md records what the module found.
"""
import numpy as np
import pytest
import torch

import metatree_edge_cases as ec
import metatree_oracle as orc
from test_gpu_metatree import _lml_scale

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
REAL = (orc.NORMAL, orc.EXPONENTIAL)
MODES = {orc.BERNOULLI: ("proba", "class"), orc.CATEGORICAL: ("proba", "class"), orc.POISSON: ("mean",),
         orc.EXPONENTIAL: ("mean",), orc.NORMAL: ("mean", "var")}


def _engine(case, state=None):
    from bayesml_amd import _mtree
    eng = _mtree.MtreePass(_mtree.FlatForest(**case["tabs"]), case["fam"], case["degree"], case["dim_cont"], case["dim_cat"],
                           case["cat_card"], case["h0"], torch.device("cuda", 0))
    eng.set_state(case["state"] if state is None else state)
    return eng


def _update(eng, case, xdtype=np.float64, kdtype=np.int64):
    xc, xk = eng.adopt_x(None if case["xc"] is None else case["xc"].astype(xdtype),
                         None if case["xk"] is None else case["xk"].astype(kdtype))
    n, bad = eng.update(xc, xk, eng.adopt_y(case["y"]))
    assert (n, bad) == (len(case["y"]), 0), case["name"]
    return eng.get_state()


def _args(case, state=None):
    return (case["tabs"], case["state"] if state is None else state, case["fam"], case["degree"], case["h0"], case["dim_cont"],
            case["xc"], case["xk"], case["y"])


def _judge(case, got, state=None, eng=None, mixture=True):
    """``got`` against the exact update of ``state``: post per node and column against e_plain, the counts, and (with
    ``mixture``) g, lml, lcm and prob in the metrics of test_gpu_metatree.py.  Returns (exact state, worst err / bound)."""
    fam = case["fam"]
    want, counts = orc.batch_update(*_args(case, state))
    plain = orc.plain_update(*_args(case, state))
    sc = orc.m_scales(case["tabs"], case["state"] if state is None else state, case["dim_cont"], case["xc"], case["xk"],
                      case["y"]) if fam == orc.NORMAL else None
    errs, bounds = orc.node_errs(fam, got["post"], want["post"], sc), orc.post_bounds(fam, plain["post"], want["post"], sc)
    if eng is not None:
        assert np.array_equal(eng.last_stats()[0][:, 0], counts), case["name"]
    worst = 0.0
    for c in range(errs.shape[1]):
        if c in bounds:
            e = float(errs[:, c].max())
            print(f"{case['name']}: post[:, {c}] worst node {int(errs[:, c].argmax())} err {e:.3e} bound {bounds[c]:.3e} "
                  f"(x{e / bounds[c]:.3g})")
            worst = max(worst, e / bounds[c])
        else:
            assert not errs[:, c].any(), (case["name"], "integer column", c, np.flatnonzero(errs[:, c]))
    assert worst <= 1.0, (case["name"], "post", worst)
    if mixture:
        seen = ~np.isnan(want["lml"])
        assert np.array_equal(np.isnan(got["lml"]), ~seen), case["name"]
        scale = max(1.0, _lml_scale(fam, want["post"][seen]))
        lml = float(np.max(np.abs(got["lml"][seen] - want["lml"][seen]))) / scale
        lcm = float(np.max(np.abs(got["lcm"] - want["lcm"]))) / scale
        g, prob = orc.log_odds_err(got["g"], want["g"]) / scale, orc.ln_prob_err(got["prob"], want["prob"]) / scale
        slack = 64 * EPS
        print(f"{case['name']}: lml {lml:.3e} lcm {lcm:.3e} g {g:.3e} prob {prob:.3e} of scale {scale:.3e}; bound {slack:.3e}")
        assert max(lml, lcm, g, prob) <= slack, case["name"]
        assert orc.fixed_points_kept(case["state"]["g"] if state is None else state["g"], got["g"]), case["name"]
        worst = max(worst, max(lml, lcm, g, prob) / slack)
    return want, worst


# ---- conditioning of the real columns -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", REAL)
@pytest.mark.parametrize("kind", ec.CONDITIONING)
@pytest.mark.parametrize("seed", [0, 1])
def test_conditioning_of_the_real_columns(kind, fam, seed):
    """(a) level 1e6, (b) row 0 an outlier alone in its leaf, (c) a scale per leaf, (d) a constant leaf, and (e) a second
    update of 50 rows on the posterior the first one left (the oracle starts from the engine's own first posterior)."""
    case = ec.conditioning(kind, fam, seed=seed)
    eng = _engine(case)
    got = _update(eng, case)
    _judge(case, got, eng=eng, mixture=False)
    second = ec.conditioning(kind, fam, n=50, seed=seed + 10)
    got2 = _update(eng, second)
    _judge(second, got2, state=got, eng=eng, mixture=False)


@pytest.mark.parametrize("fam", [orc.NORMAL, orc.EXPONENTIAL, orc.POISSON])
def test_own_rows_at_inner_nodes(fam):
    """(f) NaN rows stop at the root and at depth-1 nodes: the n_own > 0 term of the merge."""
    case = ec.nan_rows(fam)
    eng = _engine(case)
    got = _update(eng, case)
    _judge(case, got, eng=eng)
    si = eng.last_stats()[0]
    assert si[0, 0] == len(case["y"]) and si[1, 0] + si[2, 0] == len(case["y"]) - case["claims"]["own_root"]
    assert si[3:7, 0].sum() == si[1, 0] + si[2, 0] - case["claims"]["own_d1"] > 0


# ---- the mixture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [orc.BERNOULLI, orc.NORMAL])
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("g0", ec.G0, ids=[repr(g) for g in ec.G0])
def test_mixture_fixed_points_and_far_ends(fam, sign, g0):
    """An inner node's h_g at 0, 1, next to them and in between, with t far below -745 and far above 745.  What the parent
    took for the node (lcm), the parent's h_g and prob are held to the exact oracle; 0 and 1 come back bit-identical; the
    tree with prior 0 stays at exactly 0 and the tree that ends more than 745 below the others gets 0, with no NaN."""
    case = ec.mixture(fam, g0, sign)
    got = _update(_engine(case), case)
    want, _ = _judge(case, got)
    for k in ("g", "lcm", "prob"):
        assert not np.isnan(got[k]).any(), k
    if g0 in (0.0, 1.0):
        for v in (1, 2, 15, 16, 22, 23):
            assert got["g"][v] == g0
        # the node's L is its own lml at 0 and the sum of its children's L at 1 (exactly: nothing is mixed)
        assert got["lcm"][1] == (got["lml"][1] if g0 == 0.0 else got["lcm"][3] + got["lcm"][4])
    assert got["prob"][2] == 0.0 and got["prob"][1] == 0.0 and want["prob"][1] == 0.0
    assert 0.0 < got["prob"][0] < 1.0 and 0.0 < got["prob"][3] < 1.0


# ---- limits and table edges ---------------------------------------------------------------------------------------------------
def test_sixteen_way_continuous_node():
    """Rows on every threshold, +-inf, -0.0 and NaN at a node with 16 children, read as float64 and as float32."""
    case = ec.wide_continuous()
    ref = None
    for dt in (np.float64, np.float32):
        eng = _engine(case)
        got = _update(eng, case, xdtype=dt)
        _judge(case, got, eng=eng)
        xc, _ = eng.adopt_x(case["xc"].astype(dt), None)
        assert np.array_equal(eng.paths(xc, None), orc.route(case["tabs"], 1, case["xc"], None))
        ref = ref or got
        for k in orc.STATE:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (k, dt)


@pytest.mark.parametrize("card", [16, 20])
def test_sixteen_way_categorical_node(card):
    """A categorical node with 16 children read as u8, i32 and i64; with cat_card = 20 the values 16..19 match no child: the
    row stops at the node and ``bad`` stays 0 (``_update`` asserts it)."""
    case = ec.wide_categorical(card)
    ref = None
    for dt in (np.uint8, np.int32, np.int64):
        eng = _engine(case)
        got = _update(eng, case, kdtype=dt)
        _judge(case, got, eng=eng)
        si = eng.last_stats()[0]
        assert si[0, 0] - si[1:, 0].sum() == case["claims"]["outside"] == (0 if card == 16 else int((case["xk"] >= 16).sum()))
        ref = ref or got
        for k in orc.STATE:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (k, dt)


def _predictions(eng, case, state, label):
    """Every read-out of the family on the case's rows against the float64 oracle; returns the worst err / bound."""
    from bayesml_amd import _mtree
    code = dict(mean=_mtree.PRED_MEAN, proba=_mtree.PRED_PROBA, var=_mtree.PRED_VAR)
    xc, xk = eng.adopt_x(case["xc"], case["xk"])
    fam, worst = case["fam"], 0.0
    a = (case["tabs"], state, fam, case["degree"], case["dim_cont"], case["xc"], case["xk"])
    for mode in MODES[fam]:
        if mode == "class":
            continue
        got, f64, ld = eng.predict(xc, xk, code[mode]), orc.predict(*a, mode), orc.predict_ld(*a, mode)
        assert got.shape == f64.shape and np.array_equal(np.isnan(got), np.isnan(f64)), (label, mode)
        bound = 4 * orc.entry_err(f64, ld) + 64 * EPS
        ratio = float(np.max(orc.entry_err(got, f64) / bound))
        print(f"{label} {mode}: worst err / (4 e64 + 64 eps) = {ratio:.3g}; e64 max {float(np.nanmax(orc.entry_err(f64, ld))):.3e}, "
              f"NaN entries {int(np.isnan(f64).sum())}")
        assert ratio <= 1.0, (label, mode)
        worst = max(worst, ratio)
        if mode == "proba":
            cls = eng.predict(xc, xk, _mtree.PRED_CLASS)
            top = np.sort(f64, axis=1)
            clear = top[:, -1] - top[:, -2] > 2 * bound.max(axis=1) * top[:, -1]
            print(f"{label} class: {clear.mean():.3f} of the rows have a clear margin")
            assert clear.mean() >= 0.9 and np.array_equal(cls[clear], np.argmax(f64, axis=1)[clear]), label
            assert cls.dtype == np.int64 and cls.min() >= 0 and cls.max() < f64.shape[1]
    return worst


@pytest.mark.parametrize("n_nodes", [361, 362])
def test_categorical_degree_16_across_the_lds_edge(n_nodes):
    """17 integer columns: 361 nodes (6137 slots) reduce in LDS, 362 (6154) in global scratch; update, PROBA and CLASS."""
    case = ec.lds_edge(orc.CATEGORICAL, n_nodes, degree=16)
    assert case["claims"]["lds"] == (n_nodes == 361)
    eng = _engine(case)
    got = _update(eng, case)
    want, _ = _judge(case, got, eng=eng)
    assert np.array_equal(eng.last_stats()[0][0, 1:], np.bincount(case["y"], minlength=16))
    _predictions(eng, case, got, case["name"])


@pytest.mark.parametrize("n_nodes", [2048, 2049])
def test_poisson_at_the_lds_edge_itself(n_nodes):
    """3 columns: 2048 nodes fill exactly MTREE_LDS_SLOTS (the <= case, LDS), 2049 take global scratch."""
    case = ec.lds_edge(orc.POISSON, n_nodes)
    assert case["claims"]["lds"] == (n_nodes == 2048) and len(case["tabs"]["feat"]) == n_nodes
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


@pytest.mark.parametrize("fam", [orc.BERNOULLI, orc.NORMAL])
def test_depth_24_chain(fam):
    """49 nodes, 24 levels: update, the paths table and every read-out, with rows that reach the deepest leaf."""
    case = ec.deep_chain(fam)
    assert case["claims"]["deepest"] >= 5
    eng = _engine(case)
    got = _update(eng, case)
    _judge(case, got, eng=eng)
    xc, _ = eng.adopt_x(case["xc"], None)
    paths = eng.paths(xc, None)
    assert paths.shape == (1, len(case["y"]), 25) and np.array_equal(paths, orc.route(case["tabs"], 1, case["xc"], None))
    assert (paths[0, :, 24] == 48).sum() == case["claims"]["deepest"]
    _predictions(eng, case, got, case["name"])


def test_1024_trees():
    case = ec.many_trees()
    eng = _engine(case)
    got = _update(eng, case)
    _judge(case, got, eng=eng)
    _predictions(eng, case, got, case["name"])


# ---- the global-scratch table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [orc.POISSON, orc.NORMAL])
def test_global_scratch_entries_rewritten_every_round(fam):
    """4096 rows on four leaves of a depth-11 tree (and on the root and two depth-1 nodes): every 64-row round of a wave adds
    to entries that another lane of it wrote the round before.  Integer columns exact, real columns per node against
    e_plain, and two runs bit-equal."""
    from bayesml_amd import _mtree
    case = ec.rewrite(fam)
    assert len(case["tabs"]["feat"]) * 2 > _mtree.LDS_SLOTS
    eng = _engine(case)
    got = _update(eng, case)
    _judge(case, got, eng=eng)
    assert (eng.last_stats()[0][:, 0] > 0).sum() == 1 + 2 + 10 * 4          # the root, two depth-1 nodes, four paths below
    eng2 = _engine(case)
    again = _update(eng2, case)
    for k in orc.STATE:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    for a, b in zip(eng.last_stats(), eng2.last_stats()):
        assert np.array_equal(a, b)


# ---- slabs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", [orc.BERNOULLI, orc.NORMAL])
def test_64_slabs_with_empty_ones(fam):
    """n = 65537: 64 slabs of 1088 rows, of which slabs 61..63 hold no row."""
    from bayesml_amd import _mtree
    case = ec.slabs(fam, 65537)
    ni, nr, _ = _mtree.stat_cols(fam)
    assert _mtree.slabs_for(65537, 7, ni + min(nr, 1)) == 64
    spans = ec.slab_spans(65537, 64)
    assert spans[60][1] == 65537 > spans[60][0] and all(lo == hi for lo, hi in spans[61:])
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)


@pytest.mark.parametrize("fam", [orc.BERNOULLI, orc.NORMAL])
@pytest.mark.parametrize("n,S", [(65, 64), (5000, 1)])
def test_forced_slab_counts(monkeypatch, fam, n, S):
    """64 slabs for 65 rows (one full wave, one row, 62 empty slabs) and one slab for 5000 rows: the integer tables equal the
    default run's, the real columns stay within the metric."""
    from bayesml_amd import _mtree
    case = ec.slabs(fam, n)
    eng = _engine(case)
    _judge(case, _update(eng, case), eng=eng)
    default = eng.last_stats()[0]
    assert _mtree.slabs_for(n, 7, 2) != S
    monkeypatch.setattr(_mtree, "slabs_for", lambda *a: S)
    forced = _engine(case)
    got = _update(forced, case)
    _judge(case, got, eng=forced)
    assert np.array_equal(forced.last_stats()[0], default)
    if fam == orc.BERNOULLI:
        assert np.array_equal(got["post"], eng.get_state()["post"])


# ---- predict on hand-set states -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("fam,degree", [(orc.BERNOULLI, 0), (orc.CATEGORICAL, 16), (orc.CATEGORICAL, 3), (orc.POISSON, 0),
                                        (orc.EXPONENTIAL, 0), (orc.NORMAL, 0)])
def test_predict_on_hand_set_states(fam, degree, n):
    """Block edges, rows that stop at inner nodes, h_g = 0 and 1 on the paths, a tree with probability 0, NaN node values."""
    case = ec.predict_case(fam, n, degree)
    eng = _engine(case)
    _predictions(eng, case, case["state"], case["name"])
    if n == 257 and fam in (orc.EXPONENTIAL, orc.NORMAL):
        mode = "mean" if fam == orc.EXPONENTIAL else "var"
        want = orc.predict(case["tabs"], case["state"], fam, degree, 2, case["xc"], None, mode)
        assert 0 < np.isnan(want).sum() < n          # (the NaN pattern itself is compared in _predictions)


@pytest.mark.parametrize("n", [1, 257])
def test_class_ties_go_to_class_0(n):
    """Symmetric beta posteriors: both class probabilities are 1/2 at every node, every row is a tie."""
    from bayesml_amd import _mtree
    case = ec.predict_case(orc.BERNOULLI, n, symmetric=True)
    eng = _engine(case)
    xc, _ = eng.adopt_x(case["xc"], None)
    proba = eng.predict(xc, None, _mtree.PRED_PROBA)
    assert np.array_equal(proba[:, 0], proba[:, 1])
    assert not eng.predict(xc, None, _mtree.PRED_CLASS).any()
