"""``metatree.LearnModel.calc_pred_logpdf`` and ``mtpred_logpdf`` (include/mtpred.h) on the MI355X against the 50-digit
evaluation of the definition (tests/metatree_logpdf_exact.py) at tile, wave-split, depth, budget and share-threshold edges.

Bound: |lnp_i - exact_i| <= C eps (1 + M_i), M_i the largest log-term of row i, C = 4 x the worst ratio of the same
formulas in binary64 NumPy over these very cases (``ex.C``; tests/test_metatree_logpdf.py measures it without a GPU).
Every test prints its worst ratio beside C.
"""
import math

import numpy as np
import pytest
import torch

import metatree_lr_cases as lc
import metatree_logpdf_exact as ex

pytestmark = pytest.mark.gpu
FAMILIES = range(6)


def device_lnp(case, total=False, rows=None):
    from bayesml_amd import _mtpred, _mtree
    eng = _mtree.MtreePass(_mtree.FlatForest(**case["flat"]), case["fam"], case["D"], case["dim_cont"], case["dim_cat"],
                           case["cat_card"], np.zeros(1), torch.device("cuda", 0))
    eng.set_state(case["state"])
    pick = (lambda a: a if a is None or rows is None else a[rows])          # noqa: E731
    xc, xk = eng.adopt_x(pick(case["xc"]), pick(case["xk"]))
    lnp, tot = _mtpred.LogpdfPass(eng).run(xc, xk, eng.adopt_y(pick(case["y"])), total=total)
    return (lnp.cpu().numpy(), float(tot.cpu()[0])) if total else lnp.cpu().numpy()


def judge(case, got, what):
    exact, M = ex.evaluate(case, ex.MP)
    r = ex.ratios(got, exact, M)
    print(f"{what}: worst |err| / (eps (1 + M)) = {r.max():.3f} at row {r.argmax()} (C = {ex.C}), max M = {M.max():.3g}")
    assert r.max() <= ex.C, (what, float(r.max()))
    return M


@pytest.mark.parametrize("n,B,depth,dtype", ex.GRID)
@pytest.mark.parametrize("fam", FAMILIES)
def test_families_against_the_exact_reference(fam, n, B, depth, dtype):
    case = ex.grid_case(fam, n, B, depth, dtype)
    judge(case, device_lnp(case), f"family {fam} n {n} B {B} depth {depth} {np.dtype(dtype).name}")


def test_a_tile_past_the_lds_budget_is_read_where_it_lies():
    from bayesml_amd import _mtpred
    case = ex.grid_case(ex.NORMAL, 65, 5, 3, np.float32, dim_cont=65)
    assert not _mtpred.staged(65, 1) and _mtpred.staged(63, 1)
    got = device_lnp(case)
    judge(case, got, "direct form")
    narrow = dict(case, xc=case["xc"][:, :2].copy(), dim_cont=2)             # the trees read x0 and x1 only
    narrow["flat"] = dict(case["flat"], feat=np.where(case["flat"]["feat"] == 65, 2, case["flat"]["feat"]))
    assert np.array_equal(device_lnp(narrow), got)                            # staged and direct: the same bits


@pytest.mark.parametrize("fam", FAMILIES)
def test_fixed_points(fam):
    """g = 0 gives the node's own value and g = 1 the child's, bit for bit; a tree of weight 0 changes nothing."""
    n = 64
    xc = np.random.default_rng(fam).uniform(-4, 4, (n, 2))
    xc[:, 0] = np.where(np.arange(n) < 32, -1.0, 1.0) * np.abs(xc[:, 0])
    case = ex.make(fam, [lc.STUMP], xc, None, [], seed=40 + fam)
    case["state"]["prob"][:] = 1.0
    alone = lambda v: dict(case, flat=lc.forest([None]), state={k: (a[v:v + 1] if k != "prob" else a)      # noqa: E731
                                                               for k, a in case["state"].items()})
    own, left, right = (device_lnp(alone(v)) for v in range(3))
    for g, want in ((0.0, own), (1.0, np.where(xc[:, 0] < 0, left, right))):
        case["state"]["g"][0] = g
        assert np.array_equal(device_lnp(case), want), (fam, g)
    two = dict(case, flat=lc.forest([lc.STUMP, lc.full_binary(2)]))
    two["state"] = {k: np.concatenate([a, a[:1].repeat(7, 0)]) for k, a in case["state"].items()}
    two["state"]["prob"] = np.array([1.0, 0.0])
    assert np.array_equal(device_lnp(two), device_lnp(case))


@pytest.mark.parametrize("fam,y,bad", [(ex.POISSON, 10 ** 6, -1), (ex.EXPONENTIAL, 1e300, -1.0), (ex.NORMAL, 1e8, None),
                                       (ex.LINREG, 1e8, None), (ex.BERNOULLI, None, 2), (ex.CATEGORICAL, None, 3)])
def test_tails_and_labels_outside_the_support(fam, y, bad):
    """Labels at which the density underflows to 0 keep a finite lnp inside the bound; outside the support lnp = -inf."""
    xc = np.random.default_rng(3).uniform(-4, 4, (66, 2))
    case = ex.make(fam, [lc.STUMP, None, lc.full_binary(2)], xc, None, [], seed=50 + fam, alpha=(40.0, 50.0))
    if y is not None:
        if fam >= ex.NORMAL:           # |y - m| = 1e8 / sqrt(lambda) about the root's location
            c = ex.node_consts(ex.F64, fam, case["D"], case["state"]["post"][0])[0]
            loc, lam = (c[0], c[1] * (2 * c[2] - 1)) if fam == ex.NORMAL else (xc @ np.array(c[0], float), c[2] * (2 * c[3] - 1))
            case["y"] = loc + y / np.sqrt(float(lam)) * np.where(np.arange(66) % 2, 1.0, -1.0)
        else:
            case["y"] = np.full(66, y)
        got = device_lnp(case)
        assert np.all(np.isfinite(got)) and np.all(np.exp(got) == 0.0), (got.min(), got.max())
        judge(case, got, f"tail of family {fam}")
    if bad is not None:
        case["y"] = np.where(np.arange(66) % 3 == 0, bad, 1).astype(case["y"].dtype)
        got = device_lnp(case)
        assert np.all(np.isneginf(got[::3])) and np.all(np.isfinite(np.delete(got, np.s_[::3])))


@pytest.mark.parametrize("D", [1, 4, 15])
def test_linear_regression_on_both_paths(D):
    """A sixteen-way categorical root over four-way splits of x0.  Tile 0: the children hold SHARE - 1, SHARE and at most
    three lanes; tile 1: all 64 lanes in one child; tile 2: 64 distinct stop nodes at depth 2."""
    from bayesml_amd import _mtpred
    S = _mtpred.SHARE
    case = ex.paths_case(D, S)
    child, xc = case["xk"][:, 0], case["xc"]
    assert [int((child[:64] == c).sum()) for c in (0, 1)] == [S - 1, S] and np.bincount(child[:64])[2:].max() < S - 1
    paths = ex.orc.route(case["flat"], D, xc, case["xk"])[0]
    assert len(set(paths[128:, 2])) == 64 and paths[:, 2].min() > 16
    got = device_lnp(case)
    judge(case, got, f"linear regression D {D}")
    # tile 1's first SHARE - 1 rows alone: every node, the root too, has too few lanes for the matrix pipe
    few = device_lnp(case, rows=np.arange(64, 64 + S - 1))
    judge({k: (v[64:64 + S - 1] if k in ("xc", "xk", "y") else v) for k, v in case.items()}, few, f"the same rows, {S - 1} lanes")


@pytest.mark.parametrize("name", ["bernoulli", "categorical", "poisson", "exponential", "normal", "linearregression"])
def test_against_the_existing_read_outs(name):
    """Through the model: exp(lnp) against ``predict_proba`` (classifiers) and ``calc_pred_density`` (all) at ordinary
    labels, relative, within C eps (1 + M)."""
    import importlib
    from bayesml_amd import metatree
    sub = importlib.import_module("bayesml_amd." + name)
    fam = ["bernoulli", "categorical", "poisson", "exponential", "normal", "linearregression"].index(name)
    consts = {"c_degree": 3} if fam == ex.CATEGORICAL else {"c_degree": 1} if fam == ex.LINREG else {}
    leaf = lambda d: metatree._Node(d, sub_model=sub.LearnModel(**consts), leaf=True)      # noqa: E731
    right = metatree._Node(1, k=1, sub_model=sub.LearnModel(**consts), children=[leaf(2), leaf(2)])
    root = metatree._Node(0, k=0, sub_model=sub.LearnModel(**consts), children=[leaf(1), right], thresholds=np.array([-3.0, 0.0, 3.0]))
    m = metatree.LearnModel(1, 1, c_max_depth=2, SubModel=sub, sub_constants=consts, h0_metatree_list=[root], device="cuda:0")
    rng = np.random.default_rng(70 + fam)
    x, k = rng.uniform(-3, 3, (300, 1)), rng.integers(0, 2, (300, 1))
    y = ex.labels(fam, 3, 300, rng) + (1e-3 if fam == ex.EXPONENTIAL else 0)
    m.update_posterior(x[:200], k[:200], y[:200], alg_type="given_MT")
    kept = m.calc_pred_dist(x[:7], k[:7])._p_x
    lnp, tot = m.calc_pred_logpdf(x[200:], k[200:], y[200:], total=True)
    assert m._p_x is kept and lnp.dtype == np.float64 and lnp.shape == (100,)
    case = dict(fam=fam, D=consts.get("c_degree", 0), flat=m._hn.flat.arrays(), state=m._eng().get_state(), dim_cont=1, xc=x[200:],
                xk=k[200:], y=y[200:])
    M = judge(case, lnp, f"model, {name}")
    tol = ex.C * ex.EPS * (1 + M)
    dens = m.calc_pred_dist(x[200:], k[200:]).calc_pred_density(y[200:])
    e_dens = np.abs(np.expm1(lnp - np.log(dens)))
    print(f"model, {name}: exp(lnp) against calc_pred_density, worst {np.max(e_dens / tol):.3f} of the bound")
    assert np.all(e_dens <= tol)
    if fam <= ex.CATEGORICAL:
        proba = m.predict_proba(x[200:], k[200:])[np.arange(100), y[200:]]
        e_proba = np.abs(np.exp(lnp) - proba) / proba
        print(f"model, {name}: exp(lnp) against predict_proba, worst {np.max(e_proba / tol):.3f} of the bound")
        assert np.all(e_proba <= tol)
    assert abs(tot - math.fsum(lnp)) <= 100 * ex.EPS * np.abs(lnp).max()
    t_lnp, t_tot = m.calc_pred_logpdf(torch.from_numpy(x[200:]).cuda(), torch.from_numpy(k[200:]).cuda(), torch.from_numpy(y[200:]).cuda(),
                                      total=True)
    assert t_lnp.is_cuda and np.array_equal(t_lnp.cpu().numpy(), lnp) and float(t_tot) == tot


@pytest.mark.parametrize("fam", FAMILIES)
def test_total_determinism_and_row_subsets(fam):
    case = ex.grid_case(fam, 257, 9, 3)
    lnp, tot = device_lnp(case, total=True)
    again, tot2 = device_lnp(case, total=True)
    assert np.array_equal(lnp, again, equal_nan=True) and (tot == tot2 or (tot != tot and tot2 != tot2))
    fin = np.isfinite(lnp)
    if fin.all():
        assert abs(tot - math.fsum(lnp)) <= 257 * ex.EPS * np.abs(lnp).max()
    if fam != ex.LINREG:
        rows = np.r_[3:40, 100:257:3]
        assert np.array_equal(device_lnp(case, rows=rows), lnp[rows], equal_nan=True)
