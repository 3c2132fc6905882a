"""Oracle of the meta-tree forest with SubModel=linearregression (TEST INFRASTRUCTURE ONLY).

The batch form is metatree_oracle's (same walk, same mixture) with a Bayesian linear regression in every node.  With Z the
rows of R_v (the batch rows whose walk passes node v), X their continuous features and (Lambda0, mu0, alpha0, beta0, n0) the
node's current posterior:

    Lambda = Lambda0 + X'X,  mu = Lambda^-1 (X'y + Lambda0 mu0),  alpha = alpha0 + |R_v| / 2,
    beta = beta0 + (y'y + mu0'Lambda0 mu0 - mu'Lambda mu) / 2,  n = n0 + |R_v|,
    lml = a ln b - alpha ln beta + lnGamma(alpha) - lnGamma(a) + (ln|Lambda_h0| - ln|Lambda| - n ln 2 pi) / 2.

``batch_update`` evaluates this in mpmath at 50 digits (a product of two binary64 numbers has 106 bits and is exact there)
and rounds once.  ``plain_update`` restates the reference's per-node float64 formulas (``x.T @ x``, ``np.linalg.solve``, the
beta line, ``slogdet``, ``gammaln``); its deviation from the exact state is the yardstick e_plain.  The post vector of a node
is [mu (D) | upper triangle of Lambda, row-major (D (D + 1) / 2) | alpha | beta | n]; h0 has the same layout.
"""
import mpmath as mp
import numpy as np

import metatree_oracle as orc

mp.mp.dps = 50
EPS = orc.EPS
LINREG = 5


def tri(D):
    return D * (D + 1) // 2


def post_len(D):
    return D + tri(D) + 3


def pack(mu, lam, alpha, beta, n=0):
    lam = np.asarray(lam, dtype=float)
    return np.concatenate([np.asarray(mu, dtype=float), lam[np.triu_indices(len(mu))], [alpha, beta, n]])


def unpack(vec, D):
    """(mu, symmetric Lambda, alpha, beta, n) of a post vector (float64)."""
    T = tri(D)
    lam = np.zeros((D, D))
    lam[np.triu_indices(D)] = vec[D:D + T]
    lam = lam + np.triu(lam, 1).T
    return np.array(vec[:D], dtype=float), lam, float(vec[D + T]), float(vec[D + T + 1]), float(vec[D + T + 2])


def default_h0(D):
    return pack(np.zeros(D), np.eye(D), 1.0, 1.0, 0)


# ---- exact pieces -------------------------------------------------------------------------------------------------------------
def _mpf(a):
    return [mp.mpf(float(t)) for t in np.ravel(a)]


def _unpack_mp(vec, D):
    T = tri(D)
    v = _mpf(vec)
    lam = mp.zeros(D, D)
    iu = np.triu_indices(D)
    for k, (i, j) in enumerate(zip(*iu)):
        lam[int(i), int(j)] = lam[int(j), int(i)] = v[D + k]
    return mp.matrix(v[:D]), lam, v[D + T], v[D + T + 1], v[D + T + 2]


def _lndet(lam):
    L = mp.cholesky(lam)
    return 2 * mp.fsum(mp.log(L[i, i]) for i in range(lam.rows))


def lml_exact(h0, post_v, D):
    """The log marginal likelihood formula evaluated exactly on a (binary64) post vector."""
    _, lam0, a, b, _ = _unpack_mp(h0, D)
    _, lam, alpha, beta, n = _unpack_mp(post_v, D)
    return (a * mp.log(b) - alpha * mp.log(beta) + mp.loggamma(alpha) - mp.loggamma(a)
            + (_lndet(lam0) - _lndet(lam) - n * mp.log(2 * mp.pi)) / 2)


def lml_plain(h0, post_v, D):
    """The same formula as the reference writes it, in float64 (``linearregression.calc_log_marginal_likelihood``)."""
    from scipy.special import gammaln
    _, lam0, a, b, _ = unpack(np.asarray(h0, dtype=float), D)
    _, lam, alpha, beta, n = unpack(np.asarray(post_v, dtype=float), D)
    return (a * np.log(b) - alpha * np.log(beta) + gammaln(alpha) - gammaln(a)
            + 0.5 * (np.linalg.slogdet(lam0)[1] - np.linalg.slogdet(lam)[1] - n * np.log(2 * np.pi)))


def mix_exact(g, lml, kids_L):
    """(L, new g) of an inner node: t1 = ln g + sum L_c, L = logaddexp(ln(1 - g) + lml, t1), g <- exp(t1 - L)."""
    S = mp.fsum(kids_L)
    g = mp.mpf(float(g))
    if g <= 0:
        return lml, mp.mpf(0)
    if g >= 1:
        return S, mp.mpf(1)
    t1 = mp.log(g) + S
    a = mp.log(1 - g) + lml
    mx = max(a, t1)
    L = mx + mp.log(mp.exp(a - mx) + mp.exp(t1 - mx))
    return L, mp.exp(t1 - L)


def _fold_exact(p, X, y, D):
    """The exact fold of the post vector p with the rows (X, y); returns (new post as floats, S_beta as float)."""
    mu0, lam0, alpha0, beta0, n0 = _unpack_mp(p, D)
    n = len(y)
    cols = [_mpf(X[:, j]) for j in range(D)]
    ym = _mpf(y)
    lam = lam0.copy()
    for i in range(D):
        for j in range(i, D):
            s = mp.fdot(cols[i], cols[j])
            lam[i, j] += s
            if j != i:
                lam[j, i] += s
    c = lam0 * mu0
    for i in range(D):
        c[i] += mp.fdot(cols[i], ym)
    mu = mp.lu_solve(lam, c)
    yy = mp.fdot(ym, ym)
    m0 = (mu0.T * lam0 * mu0)[0]
    m1 = (mu.T * lam * mu)[0]
    beta = beta0 + (yy + m0 - m1) / 2
    s_beta = beta0 + (yy + m0 + m1) / 2
    alpha = alpha0 + mp.mpf(n) / 2
    out = [float(t) for t in mu] + [float(lam[int(i), int(j)]) for i, j in zip(*np.triu_indices(D))]
    return np.array(out + [float(alpha), float(beta), float(n0 + n)]), float(s_beta), (mu, lam, alpha, beta, n0 + n)


def batch_update(flat, state, D, h0, dim_cont, xc, xk, y):
    """One update_posterior(alg_type='given_MT') on copies of the state tables.  Returns (new state, n per node, info) with
    info['s_beta'][v] = beta0 + (y'y + mu0'Lambda0 mu0 + mu'Lambda mu) / 2 (the scale of beta's terms) and
    info['lam_scale'][v] = |Lambda0| + sum |x_i x_j| (the scale of Lambda's), NaN / zero where no row passes."""
    st = {k: np.array(v, dtype=np.float64) for k, v in state.items()}
    rows = orc.node_rows(flat, dim_cont, xc, xk)
    X, y = np.asarray(xc, dtype=np.float64)[:, :D], np.asarray(y, dtype=np.float64)
    B, nodes = len(flat["tree_off"]) - 1, len(flat["feat"])
    counts = np.zeros(nodes, dtype=np.int64)
    info = dict(s_beta=np.full(nodes, np.nan), lam_scale=np.zeros((nodes, tri(D))))
    _, lam_h0, a, b, _ = _unpack_mp(h0, D)
    lndet0 = _lndet(lam_h0)
    iu = np.triu_indices(D)
    lnp = [mp.log(mp.mpf(float(v))) if v > 0 else mp.ninf for v in st["prob"]]
    for bt in range(B):
        lo, hi = int(flat["tree_off"][bt]), int(flat["tree_off"][bt + 1])
        L = {}
        for v in range(hi - 1, lo - 1, -1):
            if rows[v] is None:
                continue
            Xv, yv = X[rows[v]], y[rows[v]]
            counts[v] = len(yv)
            info["lam_scale"][v] = np.abs(unpack(st["post"][v], D)[1])[iu] + (np.abs(Xv).T @ np.abs(Xv))[iu]
            st["post"][v], info["s_beta"][v], (mu, lam, alpha, beta, ncum) = _fold_exact(st["post"][v], Xv, yv, D)
            lml = (a * mp.log(b) - alpha * mp.log(beta) + mp.loggamma(alpha) - mp.loggamma(a)
                   + (lndet0 - _lndet(lam) - ncum * mp.log(2 * mp.pi)) / 2)
            st["lml"][v] = float(lml)
            if flat["feat"][v] < 0:
                L[v] = lml
                continue
            kids = range(int(flat["child0"][v]), int(flat["child0"][v]) + int(flat["nchild"][v]))
            for c in kids:
                st["lcm"][c] = float(L.get(c, 0))
            L[v], gn = mix_exact(st["g"][v], lml, [L.get(c, 0) for c in kids])
            st["g"][v] = float(gn)
        lnp[bt] += L.get(lo, 0)
    mx = max(lnp)
    w = [mp.exp(t - mx) for t in lnp]
    tot = mp.fsum(w)
    st["prob"] = np.array([float(t / tot) for t in w])
    return st, counts, info


def plain_update(flat, state, D, h0, dim_cont, xc, xk, y):
    """``batch_update`` as the reference computes it: per node from that node's rows, every formula in float64 NumPy."""
    from scipy.special import gammaln
    st = {k: np.array(v, dtype=np.float64) for k, v in state.items()}
    rows = orc.node_rows(flat, dim_cont, xc, xk)
    X, y = np.asarray(xc, dtype=np.float64)[:, :D], np.asarray(y, dtype=np.float64)
    _, lam_h0, a, b, _ = unpack(np.asarray(h0, dtype=float), D)
    with np.errstate(divide="ignore"):
        lnp = np.log(st["prob"])
    for bt in range(len(flat["tree_off"]) - 1):
        lo, hi = int(flat["tree_off"][bt]), int(flat["tree_off"][bt + 1])
        L = {}
        for v in range(hi - 1, lo - 1, -1):
            if rows[v] is None:
                continue
            x, yv = X[rows[v]], y[rows[v]]
            mu0, lam0, alpha, beta, n = unpack(st["post"][v], D)
            lam = lam0 + x.T @ x
            mu = np.linalg.solve(lam, x.T @ yv + lam0 @ mu0)
            alpha += len(yv) / 2.0
            beta += (-mu @ lam @ mu + yv @ yv + mu0 @ lam0 @ mu0) / 2.0
            n += len(yv)
            lml = (a * np.log(b) - alpha * np.log(beta) + gammaln(alpha) - gammaln(a)
                   + 0.5 * (np.linalg.slogdet(lam_h0)[1] - np.linalg.slogdet(lam)[1] - n * np.log(2 * np.pi)))
            st["post"][v], st["lml"][v] = pack(mu, lam, alpha, beta, n), lml
            if flat["feat"][v] < 0:
                L[v] = lml
                continue
            kids = range(int(flat["child0"][v]), int(flat["child0"][v]) + int(flat["nchild"][v]))
            lc = np.array([L.get(c, 0.0) for c in kids])
            st["lcm"][kids.start:kids.stop] = lc
            with np.errstate(divide="ignore"):
                t1 = np.log(st["g"][v]) + lc.sum()
                L[v] = np.logaddexp(np.log(1 - st["g"][v]) + lml, t1)
            st["g"][v] = np.exp(t1 - L[v])
        lnp[bt] += L.get(lo, 0.0)
    w = np.exp(lnp - lnp.max())
    st["prob"] = w / w.sum()
    return st


# ---- deviations per node and column group -------------------------------------------------------------------------------------
def post_errs(got, want, D, info, visited):
    """Over the visited nodes, the largest deviation of every column group of ``post`` from the exact table ``want``:
    n and alpha bit-equal (0 or inf); Lambda_ij relative to |Lambda0_ij| + sum |x_i x_j|; beta relative to S_beta;
    mu as ||d mu||_inf / ||mu||_inf.  ``cond`` is the largest cond_2(Lambda) of the exact table over those nodes."""
    T = tri(D)
    out = dict(n=0.0, alpha=0.0, lam=0.0, beta=0.0, mu=0.0, cond=1.0)
    for v in np.flatnonzero(visited):
        g, w = np.asarray(got[v], dtype=float), np.asarray(want[v], dtype=float)
        if np.isnan(g).any():
            return {k: np.inf for k in out}
        out["n"] = max(out["n"], 0.0 if g[D + T + 2] == w[D + T + 2] else np.inf)
        out["alpha"] = max(out["alpha"], 0.0 if g[D + T] == w[D + T] else np.inf)
        out["lam"] = max(out["lam"], float(np.max(np.abs(g[D:D + T] - w[D:D + T]) / info["lam_scale"][v])))
        out["beta"] = max(out["beta"], abs(g[D + T + 1] - w[D + T + 1]) / info["s_beta"][v])
        scale = np.max(np.abs(w[:D]))
        d = np.max(np.abs(g[:D] - w[:D]))
        out["mu"] = max(out["mu"], 0.0 if d == 0 else d / scale if scale > 0 else np.inf)
        out["cond"] = max(out["cond"], float(np.linalg.cond(unpack(w, D)[1])))
    return out


def post_bounds(plain_errs, D, cond):
    """4 x e_plain + 64 eps per column group (section 4i's rule); mu also gets D cond_2(Lambda) eps, the forward bound of a
    backward-stable solve, without which the comparison would hang on how lucky the yardstick's own solve was."""
    b = {k: 4 * plain_errs[k] + 64 * EPS for k in ("lam", "beta", "mu")}
    b["mu"] += D * cond * EPS
    return b


def unchanged_where_unvisited(before, after, visited):
    """Nodes no row passes stay bit-identical in post, g and lml (NaN stays NaN)."""
    m = ~np.asarray(visited, dtype=bool)
    return all(np.array_equal(np.asarray(before[k])[m], np.asarray(after[k])[m], equal_nan=True) for k in ("post", "g", "lml"))


def decomposed_errs(flat, before, after, D, h0, visited):
    """The edge cases' check of everything downstream of ``post``, each step against the exact formula on the device's own
    input: lml_v against lml_exact(post_v) relative to max(1, |lml|); g, lcm and prob against the exact mixture of the
    device's own lml (g in log-odds, ln prob absolutely, lcm relative to max(1, |L|))."""
    out = dict(lml=0.0, lml_plain=0.0, g=0.0, lcm=0.0, prob=0.0, scale=1.0)
    lnp = [mp.log(mp.mpf(float(v))) if v > 0 else mp.ninf for v in before["prob"]]
    g_want, lcm_want = np.array(before["g"], dtype=float), np.array(before["lcm"], dtype=float)
    for bt in range(len(flat["tree_off"]) - 1):
        lo, hi = int(flat["tree_off"][bt]), int(flat["tree_off"][bt + 1])
        L = {}
        for v in range(hi - 1, lo - 1, -1):
            if not visited[v]:
                continue
            exact = lml_exact(h0, after["post"][v], D)
            out["lml"] = max(out["lml"], float(abs(mp.mpf(float(after["lml"][v])) - exact) / max(1, abs(exact))))
            plain = mp.mpf(float(lml_plain(h0, after["post"][v], D)))
            out["lml_plain"] = max(out["lml_plain"], float(abs(plain - exact) / max(1, abs(exact))))
            out["scale"] = max(out["scale"], float(abs(exact)))
            own = mp.mpf(float(after["lml"][v]))
            if flat["feat"][v] < 0:
                L[v] = own
                continue
            kids = range(int(flat["child0"][v]), int(flat["child0"][v]) + int(flat["nchild"][v]))
            for c in kids:
                lcm_want[c] = float(L.get(c, 0))
            L[v], gn = mix_exact(before["g"][v], own, [L.get(c, 0) for c in kids])
            g_want[v] = float(gn)
        lnp[bt] += L.get(lo, 0)
    mx = max(lnp)
    w = [mp.exp(t - mx) for t in lnp]
    prob_want = np.array([float(t / mp.fsum(w)) for t in w])
    out["g"] = orc.log_odds_err(after["g"], g_want)
    out["lcm"] = float(np.max(np.abs(after["lcm"] - lcm_want) / np.maximum(1.0, np.abs(lcm_want))))
    out["prob"] = orc.ln_prob_err(np.asarray(after["prob"], dtype=float), prob_want)
    return out


# ---- read-outs (plain float64, the reference's order of operations) -----------------------------------------------------------
def node_values(post, D, X, v):
    """(p_v(x), variance_v(x)) of node v at the rows X (ref: linearregression :722-727, :823-827)."""
    mu, lam, alpha, beta, _ = unpack(post[v], D)
    lambdas = alpha / beta / (1.0 + np.sum(X.T * np.linalg.solve(lam, X.T), axis=0))
    nu = 2.0 * alpha
    with np.errstate(divide="ignore", invalid="ignore"):
        var = nu / lambdas / (nu - 2.0) if nu > 2.0 else np.full(len(X), np.nan)
    return X @ mu, var, lambdas, nu


def predict(flat, state, D, dim_cont, xc, xk, mode):
    """mode 'mean' or 'var': the reference's folds (ref:3285-3297, 3409-3450) with row-dependent node values."""
    paths = orc.route(flat, dim_cont, xc, xk)
    X = np.asarray(xc, dtype=np.float64)[:, :D]
    B, n, D1 = paths.shape
    means, vars_ = np.zeros((B, n)), np.zeros((B, n))
    for b in range(B):
        m, s2 = np.zeros(n), np.zeros(n)
        for j in range(D1 - 1, -1, -1):
            col = paths[b][:, j]
            for v in np.unique(col[col >= 0]):
                rows = col == v
                mv, vv, _, _ = node_values(state["post"], D, X[rows], v)
                last = (paths[b][rows, j + 1] < 0) if j + 1 < D1 else np.ones(rows.sum(), bool)
                g = state["g"][v]
                mm = (1 - g) * mv + g * m[rows]
                with np.errstate(invalid="ignore"):
                    s2[rows] = np.where(last, vv, (1 - g) * ((mm - mv) ** 2 + vv) + g * ((mm - m[rows]) ** 2 + s2[rows]))
                m[rows] = np.where(last, mv, mm)
        means[b], vars_[b] = m, s2
    mix = state["prob"] @ means
    return mix if mode == "mean" else state["prob"] @ ((means - mix) ** 2 + vars_)


def pred_density(flat, state, D, dim_cont, xc, xk, y):
    from scipy import stats
    paths = orc.route(flat, dim_cont, xc, xk)
    X, y = np.asarray(xc, dtype=np.float64)[:, :D], np.asarray(y, dtype=np.float64)
    out = np.zeros(paths.shape[1])
    for b in range(paths.shape[0]):
        n, D1 = paths[b].shape
        val = np.zeros(n)
        for j in range(D1 - 1, -1, -1):
            col = paths[b][:, j]
            for v in np.unique(col[col >= 0]):
                rows = col == v
                mv, _, lambdas, nu = node_values(state["post"], D, X[rows], v)
                own = stats.t.pdf(y[rows], loc=mv, scale=1.0 / np.sqrt(lambdas), df=nu)
                last = (paths[b][rows, j + 1] < 0) if j + 1 < D1 else np.ones(rows.sum(), bool)
                g = state["g"][v]
                val[rows] = np.where(last, own, (1 - g) * own + g * val[rows])
        out += state["prob"][b] * val
    return out


feature_importances = orc.feature_importances


def initial_state(flat, D, h0, g=None, prob=None):
    """Prior posts, lml NaN, lcm 0, g (default 0.5, 0 at leaves of the maximal depth is the caller's business), prob uniform."""
    nodes, B = len(flat["feat"]), len(flat["tree_off"]) - 1
    return dict(g=np.full(nodes, 0.5) if g is None else np.array(g, dtype=float),
                post=np.tile(np.asarray(h0, dtype=float), (nodes, 1)), lml=np.full(nodes, np.nan), lcm=np.zeros(nodes),
                prob=np.full(B, 1.0 / B) if prob is None else np.array(prob, dtype=float))


# ---- the golden cases (tests/golden/make_golden_metatree_lr.py) ---------------------------------------------------------------
def flatten(roots, prob, D):
    """Breadth-first tables of ``_Node`` trees whose sub-models are linearregression learners (the reference's or
    bayesml_amd's): metatree_oracle.flatten for the structure, g, lml and lcm, and the post vectors of this family."""
    flat, state, map_leaf = orc.flatten(roots, prob, orc.EXPONENTIAL)
    posts = []
    for root in roots:
        order = [root]
        for node in order:
            s = node.sub_model
            posts.append(pack(s.hn_mu_vec, s.hn_lambda_mat, s.hn_alpha, s.hn_beta, s._n))
            if not node.leaf:
                order.extend(node.children)
    state["post"] = np.array(posts)
    return flat, state, map_leaf


_MIXED = dict(c_dim_continuous=3, c_dim_categorical=2, c_max_depth=4)
_D15 = dict(c_dim_continuous=15, c_dim_categorical=0, c_max_depth=2)
CASES = [
    dict(name="mtrf", seed=7, consts=_MIXED, D=3, stage1="MTRF", n1=3000, n2=50, np_=500),
    dict(name="threeway", seed=2, consts=orc._HAND, D=2, stage1="hand", n1=400, n2=50, np_=100),
    dict(name="d15", seed=3, consts=_D15, D=15, stage1="stump", n1=600, n2=50, np_=100),
]
READOUTS = ("predict", "pred_var", "pred_density", "feature_importances")


def case_forest(case):
    """(flat, g, prob) of a case whose stage 1 replays a given forest; None for MTRF."""
    if case["stage1"] == "hand":
        flat, g = orc._hand_forest()
        return flat, g, np.array([0.4, 0.6])
    if case["stage1"] == "stump":
        flat = dict(tree_off=np.array([0, 3], np.int32), feat=np.array([0, -1, -1], np.int32),
                    child0=np.array([1, 0, 0], np.int32), nchild=np.array([2, 0, 0], np.int32),
                    thr_off=np.array([0, -1, -1], np.int32), depth=np.array([0, 1, 1], np.int32),
                    thr=np.array([-3.0, 0.0, 3.0]))
        return flat, np.array([0.5, 0.5, 0.5]), np.array([1.0])
    return None


def case_inputs(case):
    """Stage 1, stage 2 and read-out samples of a case from its seed: noise sd 1, features centred in (-3, 3) apart from
    the intercept (the last regressor when D >= 3), y piecewise linear in the features the forests route on."""
    rng = np.random.default_rng(case["seed"])
    dc, dk, D = case["consts"]["c_dim_continuous"], case["consts"]["c_dim_categorical"], case["D"]
    card = 3 if case["stage1"] == "hand" else 2
    # a centred signal of the noise's size: S_beta / beta stays below 10 even at a leaf of a handful of rows
    theta = np.linspace(0.15, -0.15, D)
    out = {}
    for tag, n in (("1", case["n1"]), ("2", case["n2"]), ("p", case["np_"])):
        xc = rng.uniform(-3, 3, size=(n, dc))
        if D >= 3:
            xc[:, -1] = 1.0
        xk = rng.integers(0, card, size=(n, dk))
        if case["stage1"] == "hand":
            xc[::7, 0] = -1.0
            xc[3::11, 0] = 1.0
        y = (xc @ theta + 0.8 * (xc[:, 0] > 0) - 0.25 + (0.4 * (xk[:, 0] - 0.5) if dk else 0.0) + rng.standard_normal(n))
        out["xc" + tag], out["xk" + tag], out["y" + tag] = xc, xk.astype(np.int64), y
    return out


def drive(module, lr_module, case, inp, forest=None):
    """Run a case through ``module.LearnModel`` (the reference's when the fixtures are made).  ``forest`` = (flat, g, prob)
    replays stage 1 as 'given_MT'.  Returns the fixture's arrays."""
    D = case["D"]
    model = module.LearnModel(SubModel=lr_module, sub_constants={"c_degree": D}, **case["consts"])
    out = {}
    forest = case_forest(case) if forest is None else forest
    if forest is not None:
        flat, g, prob = forest
        model.set_hn_params(hn_metatree_list=orc.nodes_from_flat(module, flat, g, lambda: lr_module.LearnModel(D)),
                            hn_metatree_prob_vec=np.array(prob))
        orc.widen_lcm(model)
        out["init_g"], out["init_prob"] = np.array(g, dtype=float), np.array(prob, dtype=float)
        model.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    else:
        model.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="MTRF", n_estimators=8, random_state=0)
    f1, s1, _ = flatten(model.hn_metatree_list, model.hn_metatree_prob_vec, D)
    for k in orc.STRUCT:
        out[k] = f1[k]
    for k in orc.STATE:
        out["after1_" + k] = s1[k]
    model.update_posterior(inp["xc2"], inp["xk2"], inp["y2"], alg_type="given_MT")
    _, s2, _ = flatten(model.hn_metatree_list, model.hn_metatree_prob_vec, D)
    for k in orc.STATE:
        out["after2_" + k] = s2[k]
    out["predict"] = np.asarray(model.predict(inp["xcp"], inp["xkp"]))
    model.calc_pred_dist(inp["xcp"], inp["xkp"])
    out["pred_var"] = np.asarray(model.calc_pred_var())
    out["pred_density"] = np.asarray(model.calc_pred_density(inp["yp"]))
    if case["stage1"] == "MTRF":          # (the reference adds None where a node was never visited: TypeError)
        out["feature_importances"] = np.asarray(model.calc_feature_importances(), dtype=float)
    return out


def oracle_readouts(flat, state, case, inp):
    D, dc = case["D"], case["consts"]["c_dim_continuous"]
    xk = inp["xkp"] if case["consts"]["c_dim_categorical"] else None
    out = dict(predict=predict(flat, state, D, dc, inp["xcp"], xk, "mean"),
               pred_var=predict(flat, state, D, dc, inp["xcp"], xk, "var"),
               pred_density=pred_density(flat, state, D, dc, inp["xcp"], xk, inp["yp"]))
    if case["stage1"] == "MTRF":
        out["feature_importances"] = feature_importances(flat, state, dc + case["consts"]["c_dim_categorical"])
    return out


def state_errs(st, ref):
    """g in log-odds, lml relative per array, ln prob absolutely: what ``ref_vs_batch_*`` and the fixture tests' tolerances are
    made of (``post`` is judged per column group, ``post_errs``)."""
    return dict(g=orc.log_odds_err(st["g"], ref["g"]), lml=orc.rel_err(st["lml"], ref["lml"]),
                prob=orc.ln_prob_err(st["prob"], ref["prob"]))


def error_cases(module, lr_module):
    """Boundary cases of this sub-model: name -> thunk."""
    rng = np.random.default_rng(6)
    xc, xk, y = rng.uniform(-3, 3, (20, 2)), rng.integers(0, 3, (20, 1)), rng.standard_normal(20)

    def fitted():
        flat, g = orc._hand_forest()
        m = module.LearnModel(SubModel=lr_module, sub_constants={"c_degree": 2}, **orc._HAND)
        m.set_hn_params(hn_metatree_list=orc.nodes_from_flat(module, flat, g, lambda: lr_module.LearnModel(2)))
        return orc.widen_lcm(m)

    return {
        "int_y": lambda: fitted().update_posterior(xc, xk, np.arange(20), alg_type="given_MT"),
        "wrong_shape_y": lambda: fitted().update_posterior(xc, xk, y[:5], alg_type="given_MT"),
        "y_two_dimensional": lambda: fitted().update_posterior(xc, xk, y[:, None], alg_type="given_MT"),
        "wrong_shape_x_continuous": lambda: fitted().update_posterior(xc[:, :1], xk, y, alg_type="given_MT"),
        "categorical_value_too_large": lambda: fitted().update_posterior(xc, xk + 1, y, alg_type="given_MT"),
        "pred_var_is_allowed": lambda: fitted().calc_pred_dist(xc, xk).calc_pred_var(),
        "zero_one_loss_on_regressor": lambda: fitted().calc_pred_dist(xc, xk).make_prediction(loss="0-1"),
        "density_int_y": lambda: fitted().calc_pred_dist(xc, xk).calc_pred_density(np.arange(20)),
        "given_MT_without_forest": lambda: module.LearnModel(SubModel=lr_module, sub_constants={"c_degree": 2},
                                                             **orc._HAND).update_posterior(xc, xk, y, alg_type="given_MT"),
    }
