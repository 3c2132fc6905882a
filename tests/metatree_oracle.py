"""NumPy / mpmath oracle of the meta-tree forest update and read-outs (TEST INFRASTRUCTURE ONLY), the seeded recipe of the
golden cases, and the driver that runs a case through a ``metatree`` module (the reference's when the fixtures are made,
``bayesml_amd``'s in the tests).

The batch form (ISSUE / DESIGN.md section 4i).  Let v be a node of tree b and R_v the batch rows whose walk passes v.  The
walk starts at the root; a continuous node with C children sends a row to child 0 if x < thr[1], to child C-1 if
thr[C-1] <= x, to child i if thr[i] <= x < thr[i+1]; a categorical node to child x; a row that matches no child (NaN)
stops there.  A node with empty R_v is left bit-identical and its parent takes 0.0 for it.  Otherwise the sub-model's
posterior is folded with the y of R_v, lml_v is the family's log marginal likelihood of the folded posterior (cumulative
since h0), a leaf has L_v = lml_v, an inner node t1 = ln g + sum_c L_c, L_v = logaddexp(ln(1 - g) + lml_v, t1),
g <- exp(t1 - L_v); ln p_b += L_root and prob = exp(ln p - max) normalised.

``batch_update`` evaluates this EXACTLY: statistics in integers, ``math.fsum`` and mpmath, lml and the mixture in mpmath at
50 digits, rounded to binary64 once.  The deviation of the reference's float64 recursion from it is therefore the
reference's own rounding error; the fixtures record it per case as ``ref_vs_batch_<table>`` and the GPU tests allow 4 x that +
64 eps.  The read-outs are plain float64 (``predict``, ``pred_density``, ``feature_importances``); a fixture's
``ref_vs_batch_<read-out>`` is the reference's read-out against the oracle's read-out on the oracle's exact two-stage state,
relative per array, and bounds that read-out in the same way.

Forest layout: ``_mtree.FlatForest``'s (tree_off, feat, child0, nchild, thr_off, depth, thr), nodes of a tree breadth-first;
state g, post[nodes, P], lml (NaN = never visited), lcm, prob.
"""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = np.finfo(float).eps
BERNOULLI, CATEGORICAL, POISSON, EXPONENTIAL, NORMAL = range(5)
FAMILY = {"bernoulli": BERNOULLI, "categorical": CATEGORICAL, "poisson": POISSON, "exponential": EXPONENTIAL,
          "normal": NORMAL}
STRUCT = ("tree_off", "feat", "child0", "nchild", "thr_off", "depth", "thr")
STATE = ("g", "post", "lml", "lcm", "prob")


# ---- the walk -----------------------------------------------------------------------------------------------------------------
def route(flat, dim_cont, xc, xk):
    """paths[B, n, max_depth + 1]: the nodes of every walk, root first, -1 past the stop node."""
    B = len(flat["tree_off"]) - 1
    n = len(xc) if xc is not None else len(xk)
    D = int(flat["depth"].max())
    paths = np.full((B, n, D + 1), -1, dtype=np.int64)
    rows = np.arange(n)
    for b in range(B):
        cur = np.full(n, flat["tree_off"][b], dtype=np.int64)
        alive = np.ones(n, dtype=bool)
        for d in range(D + 1):
            paths[b, alive, d] = cur[alive]
            nxt = np.full(n, -1, dtype=np.int64)
            for v in np.unique(cur[alive]):
                k, C = int(flat["feat"][v]), int(flat["nchild"][v])
                if k < 0:
                    continue
                at = alive & (cur == v)
                child = np.full(n, -1, dtype=np.int64)
                if k < dim_cont:
                    x = np.asarray(xc[:, k], dtype=np.float64)
                    t = flat["thr"][flat["thr_off"][v]:flat["thr_off"][v] + C + 1]
                    with np.errstate(invalid="ignore"):
                        child[x < t[1]] = 0
                        for i in range(1, C - 1):
                            child[(t[i] <= x) & (x < t[i + 1])] = i
                        child[t[C - 1] <= x] = C - 1
                else:
                    a = np.asarray(xk[:, k - dim_cont], dtype=np.int64)
                    ok = (a >= 0) & (a < C)
                    child[ok] = a[ok]
                go = at & (child >= 0)
                nxt[go] = flat["child0"][v] + child[go]
            alive = nxt >= 0
            cur = np.where(alive, nxt, cur)
            if not alive.any():
                break
    assert rows.size == n
    return paths


def stops(paths):
    last = (paths >= 0).sum(axis=2) - 1
    return np.take_along_axis(paths, last[:, :, None], axis=2)[:, :, 0]


# ---- the exact update ---------------------------------------------------------------------------------------------------------
def _lml(fam, h0, p, extra):
    """The family's calc_log_marginal_likelihood in mpmath; ``p`` / ``h0`` are lists of mpf, ``extra`` the cumulative n
    (normal) or sum ln y! (poisson)."""
    lg = mp.loggamma
    if fam == BERNOULLI:
        return lg(h0[0] + h0[1]) - lg(h0[0]) - lg(h0[1]) - lg(p[0] + p[1]) + lg(p[0]) + lg(p[1])
    if fam == CATEGORICAL:
        return lg(mp.fsum(h0)) - mp.fsum(lg(a) for a in h0) - lg(mp.fsum(p)) + mp.fsum(lg(a) for a in p)
    if fam == POISSON:
        return h0[0] * mp.log(h0[1]) - lg(h0[0]) - p[0] * mp.log(p[1]) + lg(p[0]) - extra
    if fam == EXPONENTIAL:
        return h0[0] * mp.log(h0[1]) - lg(h0[0]) - p[0] * mp.log(p[1]) + lg(p[0])
    return (h0[2] * mp.log(h0[3]) - p[2] * mp.log(p[3]) + lg(p[2]) - lg(h0[2])
            + (mp.log(h0[1]) - mp.log(p[1]) - extra * mp.log(2 * mp.pi)) / 2)


def _fold(fam, degree, p, ys):
    """The conjugate update of the post vector ``p`` (list of mpf) with the sample ``ys`` (exact)."""
    n = len(ys)
    if fam == BERNOULLI:
        ones = int(np.count_nonzero(ys == 1))
        return [p[0] + ones, p[1] + (n - ones)]
    if fam == CATEGORICAL:
        return [p[a] + int(np.count_nonzero(ys == a)) for a in range(degree)]
    if fam == POISSON:
        return [p[0] + int(ys.sum()), p[1] + n, p[2] + mp.fsum(mp.loggamma(int(v) + 1) for v in ys)]
    if fam == EXPONENTIAL:
        return [p[0] + n, p[1] + mp.fsum(mp.mpf(float(v)) for v in ys)]
    vals = [mp.mpf(float(v)) for v in ys]
    x_bar = mp.fsum(vals) / n
    ss = mp.fsum((v - x_bar) ** 2 for v in vals)
    m, kappa, alpha, beta, cum = p
    return [(kappa * m + n * x_bar) / (kappa + n), kappa + n, alpha + mp.mpf(n) / 2,
            beta + (ss + n * kappa / (kappa + n) * (x_bar - m) ** 2) / 2, cum + n]


def batch_update(flat, state, fam, degree, h0, dim_cont, xc, xk, y):
    """One update_posterior(alg_type='given_MT') on copies of the state tables; returns (new state, n per node)."""
    st = {k: np.array(v, dtype=np.float64) for k, v in state.items()}
    paths = route(flat, dim_cont, xc, xk)
    y = np.asarray(y)
    B, nodes = len(flat["tree_off"]) - 1, len(flat["feat"])
    counts = np.zeros(nodes, dtype=np.int64)
    h0m = [mp.mpf(float(v)) for v in h0]
    lnp = [mp.log(mp.mpf(float(v))) if v > 0 else mp.ninf for v in st["prob"]]
    for b in range(B):
        lo, hi = int(flat["tree_off"][b]), int(flat["tree_off"][b + 1])
        member = {}
        for d in range(paths.shape[2]):
            col = paths[b, :, d]
            for v in np.unique(col[col >= 0]):
                member[int(v)] = col == v
        L = {}
        for v in range(hi - 1, lo - 1, -1):
            if v not in member:
                continue
            ys = y[member[v]]
            counts[v] = len(ys)
            p = _fold(fam, degree, [mp.mpf(float(t)) for t in st["post"][v]], ys)
            extra = p[4] if fam == NORMAL else p[2] if fam == POISSON else 0
            lml = _lml(fam, h0m, p, extra)
            st["post"][v] = [float(t) for t in p]
            st["lml"][v] = float(lml)
            if flat["feat"][v] < 0:
                L[v] = lml
                continue
            kids = range(int(flat["child0"][v]), int(flat["child0"][v]) + int(flat["nchild"][v]))
            for c in kids:
                st["lcm"][c] = float(L.get(c, 0))
            S = mp.fsum(L.get(c, 0) for c in kids)
            g = mp.mpf(float(st["g"][v]))
            if g <= 0:
                L[v], gn = lml, mp.mpf(0)
            elif g >= 1:
                L[v], gn = S, mp.mpf(1)
            else:
                t1 = mp.log(g) + S
                a = mp.log(1 - g) + lml
                mx = max(a, t1)
                L[v] = mx + mp.log(mp.exp(a - mx) + mp.exp(t1 - mx))
                gn = mp.exp(t1 - L[v])
            st["g"][v] = float(gn)
        lnp[b] += L[lo]
    mx = max(lnp)
    w = [mp.exp(t - mx) for t in lnp]
    tot = mp.fsum(w)
    st["prob"] = np.array([float(t / tot) for t in w])
    return st, counts


# ---- the reference's own per-node float64 form, and deviations per node and column ------------------------------------------
def node_rows(flat, dim_cont, xc, xk):
    """rows[v]: the boolean mask of the batch rows whose walk passes node v (None where no row does)."""
    paths = route(flat, dim_cont, xc, xk)
    rows = [None] * len(flat["feat"])
    for b in range(paths.shape[0]):
        for d in range(paths.shape[2]):
            col = paths[b, :, d]
            for v in np.unique(col[col >= 0]):
                rows[int(v)] = col == v
    return rows


def _plain_lml(fam, h0, p, extra):
    """calc_log_marginal_likelihood of the scalar learners as they write it, in float64."""
    from scipy.special import gammaln
    if fam == BERNOULLI:
        return gammaln(h0[0] + h0[1]) - gammaln(h0[0]) - gammaln(h0[1]) - gammaln(p[0] + p[1]) + gammaln(p[0]) + gammaln(p[1])
    if fam == CATEGORICAL:
        return gammaln(h0.sum()) - gammaln(h0).sum() - gammaln(p.sum()) + gammaln(p).sum()
    if fam == POISSON:
        return h0[0] * np.log(h0[1]) - gammaln(h0[0]) - p[0] * np.log(p[1]) + gammaln(p[0]) - extra
    if fam == EXPONENTIAL:
        return h0[0] * np.log(h0[1]) - gammaln(h0[0]) - p[0] * np.log(p[1]) + gammaln(p[0])
    return (h0[2] * np.log(h0[3]) - p[2] * np.log(p[3]) + gammaln(p[2]) - gammaln(h0[2])
            + 0.5 * (np.log(h0[1]) - np.log(p[1]) - extra * np.log(2 * np.pi)))


def _plain_fold(fam, degree, p, ys):
    """_update_posterior of the scalar learners on the post vector p (float64), from the node's rows alone."""
    from scipy.special import gammaln
    n = ys.size
    p = p.copy()
    if fam == BERNOULLI:
        ones = np.count_nonzero(ys == 1)
        p[0] += ones
        p[1] += n - ones
    elif fam == CATEGORICAL:
        for a in range(degree):
            p[a] += np.count_nonzero(ys == a)
    elif fam == POISSON:
        p[0] += ys.sum()
        p[1] += n
        p[2] += gammaln(ys + 1).sum()
    elif fam == EXPONENTIAL:
        p[0] += n
        p[1] += ys.sum()
    else:
        x_bar = ys.sum() / n
        p[3] += (((ys - x_bar) ** 2).sum() + n * p[1] / (p[1] + n) * (x_bar - p[0]) ** 2) / 2.0
        p[0] = (p[1] * p[0] + n * x_bar) / (p[1] + n)
        p[1] += n
        p[2] += n * 0.5
        p[4] += n
    return p


def plain_update(flat, state, fam, degree, h0, dim_cont, xc, xk, y):
    """``batch_update`` as the reference computes it: per node from that node's rows, every formula in float64 numpy
    (x_bar = y.sum() / n, ((y - x_bar) ** 2).sum(), scipy's gammaln, np.logaddexp).  Its deviation from the exact state is
    what plain float64 costs on a case: the yardstick ``e_plain`` of the GPU tests."""
    st = {k: np.array(v, dtype=np.float64) for k, v in state.items()}
    rows = node_rows(flat, dim_cont, xc, xk)
    y, h0 = np.asarray(y), np.asarray(h0, dtype=np.float64)
    with np.errstate(divide="ignore"):
        lnp = np.log(st["prob"])
    for b in range(len(flat["tree_off"]) - 1):
        lo, hi = int(flat["tree_off"][b]), int(flat["tree_off"][b + 1])
        L = {}
        for v in range(hi - 1, lo - 1, -1):
            if rows[v] is None:
                continue
            p = _plain_fold(fam, degree, st["post"][v], y[rows[v]])
            lml = _plain_lml(fam, h0, p, p[4] if fam == NORMAL else p[2] if fam == POISSON else 0.0)
            st["post"][v], st["lml"][v] = p, lml
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
        lnp[b] += L[lo]
    w = np.exp(lnp - lnp.max())
    st["prob"] = w / w.sum()
    return st


def m_scales(flat, state, dim_cont, xc, xk, y):
    """The condition scale of a normal node's posterior mean: (kappa0 |m0| + sum_{i in R_v} |y_i|) / (kappa0 + n_v), with
    the state before the update; one per node (the prior's |m0| where no row passes)."""
    rows, y = node_rows(flat, dim_cont, xc, xk), np.asarray(y, dtype=np.float64)
    post = np.asarray(state["post"], dtype=np.float64)
    out = np.abs(post[:, 0]).copy()
    for v, r in enumerate(rows):
        if r is not None:
            out[v] = (post[v, 1] * abs(post[v, 0]) + math.fsum(np.abs(y[r]))) / (post[v, 1] + int(r.sum()))
    return out


# columns of ``post`` that hold integer values (or halves): they must be bit-equal to the exact state
INT_COLS = {BERNOULLI: (0, 1), POISSON: (0, 1), EXPONENTIAL: (0,), NORMAL: (1, 2, 4)}


def node_errs(fam, got, want, scales=None):
    """Deviations of a ``post`` table per node and per column, [nodes, P].  Integer-valued columns (bernoulli / categorical
    counts, poisson alpha and beta, exponential alpha, normal kappa, alpha and n): 0 where bit-equal, inf elsewhere.
    Columns made of non-negative terms (exponential beta, poisson sum ln y!, normal beta): |d| / |exact|.  Normal m:
    |d| / scales[node] (``m_scales``).  A NaN, or an entry that differs where the scale is 0, is inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        raise ValueError("shapes differ")
    out = np.zeros(want.shape)
    ints = range(want.shape[1]) if fam == CATEGORICAL else INT_COLS[fam]
    for c in range(want.shape[1]):
        d = np.abs(got[:, c] - want[:, c])
        if c in ints:
            out[:, c] = np.where(got[:, c] == want[:, c], 0.0, np.inf)
            continue
        den = np.abs(want[:, c]) if not (fam == NORMAL and c == 0) else np.asarray(scales, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, c] = np.where(d == 0, 0.0, np.where(den > 0, d / den, np.inf))
        out[np.isnan(d), c] = np.inf
    return out


def real_cols(fam):
    return [] if fam in (BERNOULLI, CATEGORICAL) else [c for c in range({POISSON: 3, EXPONENTIAL: 2, NORMAL: 5}[fam])
                                                       if c not in INT_COLS[fam]]


def post_bounds(fam, plain, exact, scales=None):
    """col -> 4 x e_plain + 64 eps for every real column, e_plain = max over nodes of node_errs(plain, exact)."""
    e = node_errs(fam, plain, exact, scales)
    return {c: 4 * float(e[:, c].max()) + 64 * EPS for c in real_cols(fam)}


def predict_ld(flat, state, fam, degree, dim_cont, xc, xk, mode):
    """``predict``'s fold in np.longdouble (mean, proba or var), [n] or [n, C] longdouble.  NaN node values (exponential
    alpha <= 1, normal nu <= 2) follow ``node_values``."""
    ld = np.longdouble
    paths = route(flat, dim_cont, xc, xk)
    post, g, prob = (np.asarray(state[k], dtype=np.float64).astype(ld) for k in ("post", "g", "prob"))
    one = ld(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if fam == BERNOULLI:
            th = post[:, 0] / (post[:, 0] + post[:, 1])
            V = np.stack([one - th, th], axis=1)
        elif fam == CATEGORICAL:
            V = post / post.sum(axis=1, keepdims=True)
        elif fam == POISSON:
            V = (post[:, 0] / post[:, 1])[:, None]          # alpha theta / (1 - theta), theta = 1 / (1 + beta)
        elif fam == EXPONENTIAL:
            V = np.where(post[:, 0] > 1, post[:, 1] / (post[:, 0] - one), ld(np.nan))[:, None]
        else:
            V = post[:, 0:1]
            nu, lam = 2 * post[:, 2], post[:, 1] / (post[:, 1] + one) * post[:, 2] / post[:, 3]
            S2 = np.where(nu > 2, nu / lam / (nu - 2), ld(np.nan))
    B, n = paths.shape[0], paths.shape[1]
    if mode == "var":
        means, vars_ = np.zeros((B, n), dtype=ld), np.zeros((B, n), dtype=ld)
        for b in range(B):
            m, s2 = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
            D1 = paths.shape[2]
            for j in range(D1 - 1, -1, -1):
                v = paths[b][:, j]
                valid = v >= 0
                last = valid & ((paths[b][:, j + 1] < 0) if j + 1 < D1 else True)
                m[last], s2[last] = V[v[last], 0], S2[v[last]]
                mid = valid & ~last
                gv, mv, vv = g[v[mid]], V[v[mid], 0], S2[v[mid]]
                mm = (one - gv) * mv + gv * m[mid]
                s2[mid] = (one - gv) * ((mm - mv) ** 2 + vv) + gv * ((mm - m[mid]) ** 2 + s2[mid])
                m[mid] = mm
            means[b], vars_[b] = m, s2
        mix = prob @ means
        return prob @ ((means - mix) ** 2 + vars_)
    out = np.zeros((n, V.shape[1]), dtype=ld)
    for b in range(B):
        D1 = paths.shape[2]
        val = np.zeros((n, V.shape[1]), dtype=ld)
        for j in range(D1 - 1, -1, -1):
            v = paths[b][:, j]
            valid = v >= 0
            last = valid & ((paths[b][:, j + 1] < 0) if j + 1 < D1 else True)
            val[last] = V[v[last]]
            mid = valid & ~last
            gm = g[v[mid]][:, None]
            val[mid] = (one - gm) * V[v[mid]] + gm * val[mid]
        out += prob[b] * val
    return out[:, 0] if mode == "mean" else out


def entry_err(a, ref):
    """|a - ref| / |ref| per entry (0 where equal, inf where the NaN patterns differ or ref = 0 and a does not)."""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    d = np.abs(a - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0, 0, np.where(np.abs(ref) > 0, d / np.abs(ref), np.inf))
    e = np.where(np.isnan(a) & np.isnan(ref), 0, e)
    e = np.where(np.isnan(a) != np.isnan(ref), np.inf, e)
    return e.astype(np.float64)


# ---- read-outs (plain float64, in the scalar learners' order of operations) ---------------------------------------------------
def node_values(fam, degree, post, var=False):
    """V[nodes, C] (and the variance table for normal with ``var``)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if fam == BERNOULLI:
            th = post[:, 0] / (post[:, 0] + post[:, 1])
            return np.stack([1.0 - th, th], axis=1)
        if fam == CATEGORICAL:
            return post / post.sum(axis=1, keepdims=True)
        if fam == POISSON:
            th = 1.0 / (1.0 + post[:, 1])
            return (post[:, 0] * th / (1.0 - th))[:, None]
        if fam == EXPONENTIAL:
            return np.where(post[:, 0] > 1.0, post[:, 1] / (post[:, 0] - 1.0), np.nan)[:, None]
        if not var:
            return post[:, 0:1]
        nu, lam = 2.0 * post[:, 2], post[:, 1] / (post[:, 1] + 1.0) * post[:, 2] / post[:, 3]
        return post[:, 0:1], np.where(nu > 2.0, nu / lam / (nu - 2.0), np.nan)


def fold_paths(paths_b, g, V):
    """value[n, C] of one tree: p at the stop node, (1 - g) p + g value(child) above it."""
    n, D1 = paths_b.shape
    val = np.zeros((n, V.shape[1]))
    for j in range(D1 - 1, -1, -1):
        v = paths_b[:, j]
        valid = v >= 0
        last = valid & ((paths_b[:, j + 1] < 0) if j + 1 < D1 else True)
        val[last] = V[v[last]]
        mid = valid & ~last
        gm = g[v[mid]][:, None]
        val[mid] = (1.0 - gm) * V[v[mid]] + gm * val[mid]
    return val


def predict(flat, state, fam, degree, dim_cont, xc, xk, mode):
    """mode: 'mean', 'proba', 'class' or 'var'."""
    paths = route(flat, dim_cont, xc, xk)
    B = paths.shape[0]
    if mode == "var":
        M, S2 = node_values(fam, degree, state["post"], var=True)
        means, vars_ = [], []
        for b in range(B):
            n, D1 = paths[b].shape
            m, s2 = np.zeros(n), np.zeros(n)
            for j in range(D1 - 1, -1, -1):
                v = paths[b][:, j]
                valid = v >= 0
                last = valid & ((paths[b][:, j + 1] < 0) if j + 1 < D1 else True)
                m[last], s2[last] = M[v[last], 0], S2[v[last]]
                mid = valid & ~last
                gv, mv, vv = state["g"][v[mid]], M[v[mid], 0], S2[v[mid]]
                mm = (1 - gv) * mv + gv * m[mid]
                s2[mid] = (1 - gv) * ((mm - mv) ** 2 + vv) + gv * ((mm - m[mid]) ** 2 + s2[mid])
                m[mid] = mm
            means.append(m)
            vars_.append(s2)
        means, vars_ = np.array(means), np.array(vars_)
        mix = state["prob"] @ means
        return state["prob"] @ ((means - mix) ** 2 + vars_)
    V = node_values(fam, degree, state["post"])
    vals = np.stack([fold_paths(paths[b], state["g"], V) for b in range(B)])          # [B, n, C]
    mixed = np.einsum("b,bnc->nc", state["prob"], vals)
    if mode == "mean":
        return mixed[:, 0]
    return mixed if mode == "proba" else np.argmax(mixed, axis=1)


def node_density(fam, post_v, y):
    """The predictive density of one node at the values y, as the scalar learners evaluate it."""
    from scipy import stats
    if fam == BERNOULLI:
        th = post_v[0] / (post_v[0] + post_v[1])
        return np.where(y == 1, th, 1.0 - th)
    if fam == CATEGORICAL:
        return (post_v / post_v.sum())[y]
    if fam == POISSON:
        th = 1.0 / (1.0 + post_v[1])
        return stats.nbinom.pmf(y, n=post_v[0], p=(1.0 - th))
    if fam == EXPONENTIAL:
        return stats.lomax.pdf(y, c=post_v[0], scale=post_v[1])
    lam = post_v[1] / (post_v[1] + 1) * post_v[2] / post_v[3]
    return stats.t.pdf(y, loc=post_v[0], scale=1.0 / np.sqrt(lam), df=2 * post_v[2])


def pred_density(flat, state, fam, dim_cont, xc, xk, y):
    """calc_pred_density: the fold of ``fold_paths`` with node values that depend on the row's y, mixed over trees."""
    paths = route(flat, dim_cont, xc, xk)
    y = np.asarray(y)
    out = np.zeros(paths.shape[1])
    for b in range(paths.shape[0]):
        n, D1 = paths[b].shape
        val = np.zeros(n)
        for j in range(D1 - 1, -1, -1):
            v = paths[b][:, j]
            last = (v >= 0) & ((paths[b][:, j + 1] < 0) if j + 1 < D1 else True)
            for node in np.unique(v[v >= 0]):
                rows = v == node
                own = node_density(fam, state["post"][node], y[rows])
                g = state["g"][node]
                val[rows] = np.where(last[rows], own, (1 - g) * own + g * val[rows])
        out += state["prob"][b] * val
    return out


def feature_importances(flat, state, dim_features):
    """calc_feature_importances (ref:3452-3477) on the node tables: per inner node, h_g times (the children's importances +
    at the node's feature, the children's lml minus its own), mixed over trees."""
    acc = np.zeros((len(flat["feat"]), dim_features))
    for v in range(len(flat["feat"]) - 1, -1, -1):
        if flat["feat"][v] < 0:
            continue
        kids = slice(int(flat["child0"][v]), int(flat["child0"][v]) + int(flat["nchild"][v]))
        tmp = acc[kids].sum(0)
        for c in range(kids.start, kids.stop):
            tmp[flat["feat"][v]] += state["lml"][c]
        tmp[flat["feat"][v]] -= state["lml"][v]
        acc[v] = state["g"][v] * tmp
    return sum(state["prob"][b] * acc[flat["tree_off"][b]] for b in range(len(flat["tree_off"]) - 1))


READOUTS = ("predict", "predict_proba", "pred_var", "pred_density", "feature_importances")


def oracle_readouts(flat, state, case, inp):
    """Every float read-out of a case from the state tables ``state``, by the float64 oracle."""
    fam, dc = FAMILY[case["sub"]], case["consts"]["c_dim_continuous"]
    degree = case.get("sub_constants", {}).get("c_degree", 0)
    out = {}
    if fam in (BERNOULLI, CATEGORICAL):
        out["predict_proba"] = predict(flat, state, fam, degree, dc, inp["xcp"], inp["xkp"], "proba")
    else:
        out["predict"] = predict(flat, state, fam, degree, dc, inp["xcp"], inp["xkp"], "mean")
    if fam == NORMAL:
        out["pred_var"] = predict(flat, state, fam, degree, dc, inp["xcp"], inp["xkp"], "var")
    out["pred_density"] = pred_density(flat, state, fam, dc, inp["xcp"], inp["xkp"], inp["yp"])
    if case["stage1"] == "MTRF":
        out["feature_importances"] = feature_importances(flat, state, dc + case["consts"]["c_dim_categorical"])
    return out


def readout_tols(fx):
    """4 x ref_vs_batch + 64 eps of every float read-out the fixture holds (relative per array)."""
    return {k: 4 * float(fx["ref_vs_batch_" + k]) + 64 * EPS for k in READOUTS if "ref_vs_batch_" + k in fx}


# ---- _Node trees <-> tables -------------------------------------------------------------------------------------------------
def post_of(fam, sub):
    if fam == CATEGORICAL:
        return np.array(sub.hn_alpha_vec, dtype=float)
    if fam == NORMAL:
        return np.array([sub.hn_m, sub.hn_kappa, sub.hn_alpha, sub.hn_beta, sub._n], dtype=float)
    if fam == POISSON:
        return np.array([sub.hn_alpha, sub.hn_beta, sub._sum_log_factorial], dtype=float)
    return np.array([sub.hn_alpha, sub.hn_beta], dtype=float)


def flatten(roots, prob, fam):
    """Breadth-first tables of a list of ``_Node`` trees (the reference's or bayesml_amd's)."""
    out = {k: [] for k in ("feat", "child0", "nchild", "thr_off", "depth", "thr", "g", "post", "lml", "lcm", "map_leaf")}
    tree_off = [0]
    for root in roots:
        order, base = [(root, 0.0)], len(out["feat"])
        for node, lcm in order:
            out["g"].append(float(node.h_g))
            out["post"].append(post_of(fam, node.sub_model))
            out["lml"].append(np.nan if node.log_marginal_likelihood is None else float(node.log_marginal_likelihood))
            out["lcm"].append(lcm)
            out["depth"].append(node.depth)
            out["map_leaf"].append(bool(node.map_leaf))
            if node.leaf:
                for k, v in (("feat", -1), ("child0", 0), ("nchild", 0), ("thr_off", -1)):
                    out[k].append(v)
                continue
            out["feat"].append(int(node.k))
            out["child0"].append(base + len(order))
            out["nchild"].append(len(node.children))
            if node.thresholds is not None:
                out["thr_off"].append(len(out["thr"]))
                out["thr"].extend(np.asarray(node.thresholds, dtype=float))
            else:
                out["thr_off"].append(-1)
            order.extend((c, float(node.log_children_marginal_likelihood[i])) for i, c in enumerate(node.children))
        tree_off.append(len(out["feat"]))
    flat = dict(tree_off=np.array(tree_off, np.int32), thr=np.array(out["thr"], np.float64),
                **{k: np.array(out[k], np.int32) for k in ("feat", "child0", "nchild", "thr_off", "depth")})
    state = dict(g=np.array(out["g"]), post=np.array(out["post"]).reshape(len(out["g"]), -1), lml=np.array(out["lml"]),
                 lcm=np.array(out["lcm"]), prob=np.array(prob, dtype=float))
    return flat, state, np.array(out["map_leaf"], dtype=np.uint8)


def nodes_from_flat(module, flat, g, sub_module):
    """``_Node`` trees with the structure of ``flat`` and h_g = g, default sub-models: what a caller hands to
    ``set_hn_params(hn_metatree_list=...)``."""
    roots, nodes = [], {}
    Node = getattr(module, "_Node", None) or module._metatree._Node
    for b in range(len(flat["tree_off"]) - 1):
        lo, hi = int(flat["tree_off"][b]), int(flat["tree_off"][b + 1])
        nodes[lo] = Node(0)
        for v in range(lo, hi):
            node = nodes[v]
            node.h_g = float(g[v])
            node.sub_model = sub_module()
            if flat["feat"][v] < 0:
                node.leaf = True
                continue
            node.k = int(flat["feat"][v])
            C, c0 = int(flat["nchild"][v]), int(flat["child0"][v])
            if flat["thr_off"][v] >= 0:
                node.thresholds = np.array(flat["thr"][flat["thr_off"][v]:flat["thr_off"][v] + C + 1])
            node.children = [Node(node.depth + 1) for _ in range(C)]
            for c in range(C):
                nodes[c0 + c] = node.children[c]
        roots.append(nodes[lo])
    return roots


def flatten_gen(root):
    """A GenModel's parameter tree breadth-first: structure, h_g, and the leaves' sub-model parameters (NaN rows above)."""
    out = dict(feat=[], nchild=[], depth=[], thr=[], g=[], params=[])
    order = [root]
    for node in order:
        out["depth"].append(node.depth)
        out["g"].append(float(node.h_g))
        vals = [np.ravel(v) for v in node.sub_model.get_params().values()]
        out["params"].append(np.concatenate(vals) if node.leaf else np.full(sum(len(v) for v in vals), np.nan))
        out["feat"].append(-1 if node.leaf else int(node.k))
        out["nchild"].append(0 if node.leaf else len(node.children))
        if not node.leaf:
            if node.thresholds is not None:
                out["thr"].extend(np.asarray(node.thresholds, dtype=float))
            order.extend(node.children)
    return dict(feat=np.array(out["feat"], np.int32), nchild=np.array(out["nchild"], np.int32),
                depth=np.array(out["depth"], np.int32), thr=np.array(out["thr"], np.float64), g=np.array(out["g"]),
                params=np.array(out["params"], dtype=float))


# ---- deviations ---------------------------------------------------------------------------------------------------------------
def log_odds_err(g, g_ref):
    """max (|dg| - ulp(g_ref)) / max(g (1 - g), 1e-6): the deviation in log-odds where g is at least 1e-6 from both ends,
    and the absolute deviation in units of 1e-6 nearer to them (next to 1 a comparison of log-odds means nothing: 1 - g has
    an ulp of g left, and the reference's exp(t1 - L) has lost it or rounded to 1).  One ulp of g is always allowed.  That
    the fixed points g = 0 and g = 1 are kept exactly is checked apart (``fixed_points_kept``)."""
    g, g_ref = np.asarray(g, dtype=float), np.asarray(g_ref, dtype=float)
    if g.shape != g_ref.shape or np.isnan(g).any():
        return np.inf
    excess = np.maximum(np.abs(g - g_ref) - np.spacing(g_ref), 0.0)
    return float(np.max(excess / np.maximum(g_ref * (1 - g_ref), 1e-6))) if g.size else 0.0


def fixed_points_kept(g_before, g_after):
    g_before, g_after = np.asarray(g_before), np.asarray(g_after)
    m = (g_before == 0.0) | (g_before == 1.0)
    return bool(np.array_equal(g_before[m], g_after[m]))


def rel_err(a, ref):
    """max |a - ref| / max |ref| over the finite entries of ref; the NaN pattern must agree."""
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    if a.shape != ref.shape or not np.array_equal(np.isnan(a), np.isnan(ref)):
        return np.inf
    m = ~np.isnan(ref)
    if not m.any():
        return 0.0
    scale = np.max(np.abs(ref[m]))
    return float(np.max(np.abs(a[m] - ref[m])) / scale) if scale > 0 else float(np.max(np.abs(a[m])))


def ln_prob_err(p, p_ref):
    m = p_ref > 1e-300
    if not np.array_equal(p[~m] > 1e-300, p_ref[~m] > 1e-300):
        return np.inf
    return float(np.max(np.abs(np.log(p[m]) - np.log(p_ref[m])))) if m.any() else 0.0


def state_errs(st, ref):
    """The four deviations that ``ref_vs_batch`` and the tolerances are made of."""
    return dict(g=log_odds_err(st["g"], ref["g"]), post=rel_err(st["post"], ref["post"]), lml=rel_err(st["lml"], ref["lml"]),
                prob=ln_prob_err(st["prob"], ref["prob"]))


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _hand_forest():
    """Two hand-built trees over x_continuous[0] (three-way), x_continuous[1] (binary) and x_categorical[0] (three-way).
    Tree 0: root splits x0 at -1 and 1; its middle child splits the categorical feature, its right child x1 at 0.5.
    Tree 1: root splits the categorical feature; its last child splits x0."""
    flat = dict(tree_off=np.array([0, 9, 16], np.int32),
                feat=np.array([0, -1, 2, 1, -1, -1, -1, -1, -1, 2, -1, -1, 0, -1, -1, -1], np.int32),
                child0=np.array([1, 0, 4, 7, 0, 0, 0, 0, 0, 10, 0, 0, 13, 0, 0, 0], np.int32),
                nchild=np.array([3, 0, 3, 2, 0, 0, 0, 0, 0, 3, 0, 0, 3, 0, 0, 0], np.int32),
                thr_off=np.array([0, -1, -1, 4, -1, -1, -1, -1, -1, -1, -1, -1, 7, -1, -1, -1], np.int32),
                depth=np.array([0, 1, 1, 1, 2, 2, 2, 2, 2, 0, 1, 1, 1, 2, 2, 2], np.int32),
                thr=np.array([-3.0, -1.0, 1.0, 3.0, -3.0, 0.5, 3.0, -3.0, -0.5, 0.25, 3.0]))
    g = np.where(flat["depth"] == 2, 0.0, np.where(flat["feat"] < 0, 0.5, 0.5))
    g[0], g[9] = 0.7, 0.3
    return flat, g


_MIXED = dict(c_dim_continuous=3, c_dim_categorical=2, c_max_depth=4)
_HAND = dict(c_dim_continuous=2, c_dim_categorical=1, c_max_depth=2, c_num_children_vec=np.array([3, 2, 3]),
             c_num_assignment_vec=np.array([1, -1, -1]))
CASES = [
    dict(name="bernoulli", sub="bernoulli", consts=_MIXED, stage1="MTRF", n1=3000, n2=50, np_=500),
    dict(name="categorical", sub="categorical", consts=_MIXED, sub_constants={"c_degree": 3}, stage1="MTRF", n1=3000, n2=50,
         np_=500),
    dict(name="poisson", sub="poisson", consts=_MIXED, stage1="MTRF", n1=3000, n2=50, np_=500),
    dict(name="exponential", sub="exponential", consts=_MIXED, stage1="MTRF", n1=3000, n2=50, np_=500),
    dict(name="normal", sub="normal", consts=_MIXED, stage1="MTRF", n1=3000, n2=50, np_=500),
    dict(name="normal_1e6", sub="normal", consts=_MIXED, stage1="MTRF", n1=3000, n2=50, np_=500, offset=1e6, noise=0.01),
    dict(name="threeway", sub="bernoulli", consts=_HAND, stage1="hand", n1=400, n2=50, np_=100),
    dict(name="threeway_n1", sub="poisson", consts=_HAND, stage1="hand", n1=1, n2=1, np_=3),
    dict(name="threeway_oneleaf", sub="normal", consts=_HAND, stage1="hand", n1=64, n2=5, np_=10, one_leaf=True),
]


def case_inputs(case):
    """x1 / y1 (stage 1), x2 / y2 (stage 2) and xp / yp (the read-outs) of a case, from its seed."""
    seed = sum(ord(c) for c in case["name"])
    rng = np.random.default_rng(seed)
    dc, dk = case["consts"]["c_dim_continuous"], case["consts"]["c_dim_categorical"]
    card = 3 if case["stage1"] == "hand" else 2
    fam = FAMILY[case["sub"]]
    out = {}
    for tag, n in (("1", case["n1"]), ("2", case["n2"]), ("p", case["np_"])):
        xc = rng.uniform(-3, 3, size=(n, dc))
        xk = rng.integers(0, card, size=(n, dk))
        if case["stage1"] == "hand":
            if case.get("one_leaf"):
                xc[:, 0] = rng.uniform(-2.9, -1.1, size=n)       # tree 0: child 0 of the root, a leaf
                xk[:, 0] = 0                                     # tree 1: child 0 of the root, a leaf
            else:
                xc[::7, 0] = -1.0                                # rows exactly on the thresholds: they go right
                xc[3::11, 0] = 1.0
                xc[5::13, 1] = 0.5
                mid = (xc[:, 0] >= -1.0) & (xc[:, 0] < 1.0)
                xk[mid & (xk[:, 0] == 2), 0] = 1                 # tree 0: the last child of the categorical node gets no row
        s = (xc[:, 0] > 0).astype(int) + 2 * (xc[:, 1] > 0.5) + xk[:, 0]
        if fam == BERNOULLI:
            y = (rng.random(n) < np.array([0.1, 0.3, 0.5, 0.7, 0.9, 0.95])[np.minimum(s, 5)]).astype(int)
        elif fam == CATEGORICAL:
            y = (s + rng.integers(0, 2, n)) % 3
        elif fam == POISSON:
            y = rng.poisson(1.0 + 2.0 * s)
        elif fam == EXPONENTIAL:
            y = rng.exponential(0.5 + s)
        else:
            y = case.get("offset", 0.0) + 1.0 * s + case.get("noise", 0.5) * rng.standard_normal(n)
        out["xc" + tag], out["xk" + tag], out["y" + tag] = xc, xk.astype(np.int64), y
    return out


def widen_lcm(model):
    """The reference allocates ``log_children_marginal_likelihood`` as np.zeros(2) whatever the number of children
    (ref:1376, 1615), so its own update raises IndexError at a three-way node.  When the fixtures are made, the scratch
    arrays of its trees are given their node's width first; bayesml_amd's forest is a property and is not touched."""
    for root in model.__dict__.get("hn_metatree_list", []):
        order = [root]
        for node in order:
            if not node.leaf:
                node.log_children_marginal_likelihood = np.zeros(len(node.children))
                order.extend(node.children)
    return model


def drive(module, submodules, case, inp, forest=None):
    """Run a case through ``module.LearnModel``.  ``forest`` = (flat, g, prob) replays stage 1 as 'given_MT' on a given
    forest (MTRF cases without scikit-learn); hand cases always do.  Returns the fixture's arrays."""
    fam = FAMILY[case["sub"]]
    sub = submodules[case["sub"]]
    model = module.LearnModel(SubModel=sub, sub_constants=case.get("sub_constants", {}), **case["consts"])
    out = {}
    if case["stage1"] == "hand" and forest is None:
        flat, g = _hand_forest()
        forest = (flat, g, np.array([0.4, 0.6]))
    if forest is not None:
        flat, g, prob = forest
        make_sub = lambda: sub.LearnModel(**case.get("sub_constants", {}))      # noqa: E731
        model.set_hn_params(hn_metatree_list=nodes_from_flat(module, flat, g, make_sub), hn_metatree_prob_vec=np.array(prob))
        widen_lcm(model)
        f0, s0, _ = flatten(model.hn_metatree_list, model.hn_metatree_prob_vec, fam)
        model.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="given_MT")
    else:
        model.update_posterior(inp["xc1"], inp["xk1"], inp["y1"], alg_type="MTRF", n_estimators=8, random_state=0)
    f1, s1, _ = flatten(model.hn_metatree_list, model.hn_metatree_prob_vec, fam)
    for k in STRUCT:
        out[k] = f1[k]
    if forest is not None:
        out["init_g"], out["init_prob"] = s0["g"], s0["prob"]
    for k in STATE:
        out["after1_" + k] = s1[k]
    model.update_posterior(inp["xc2"], inp["xk2"], inp["y2"], alg_type="given_MT")
    _, s2, _ = flatten(model.hn_metatree_list, model.hn_metatree_prob_vec, fam)
    for k in STATE:
        out["after2_" + k] = s2[k]
    out["predict"] = np.asarray(model.predict(inp["xcp"], inp["xkp"]))
    if fam in (BERNOULLI, CATEGORICAL):
        out["predict_proba"] = np.asarray(model.predict_proba(inp["xcp"], inp["xkp"]))
    if fam == NORMAL:
        model.calc_pred_dist(inp["xcp"], inp["xkp"])
        out["pred_var"] = np.asarray(model.calc_pred_var())
    model.calc_pred_dist(inp["xcp"], inp["xkp"])
    out["pred_density"] = np.asarray(model.calc_pred_density(inp["yp"]))
    if case["stage1"] == "MTRF":          # (the reference adds None where a node was never visited: TypeError)
        out["feature_importances"] = np.asarray(model.calc_feature_importances(), dtype=float)
    model.estimate_params(loss="0-1", visualize=False)
    if hasattr(model, "_last_map"):
        out["map_index"], out["map_leaf"] = np.int64(model._last_map[0]), np.array(model._last_map[1], dtype=np.uint8)
    else:
        trees, prob = model.hn_metatree_list, model.hn_metatree_prob_vec
        best = int(np.argmax([prob[i] * model._map_recursion(t) for i, t in enumerate(trees)]))
        out["map_index"] = np.int64(best)
        out["map_leaf"] = flatten([trees[best]], [1.0], fam)[2]
    return out


def outcome(fn):
    """The exception class name a boundary case raises, or None."""
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn()
    except Exception as e:      # noqa: BLE001
        return type(e).__name__
    return None


def error_cases(module, submodules):
    """Boundary cases: name -> thunk."""
    bern, pois = submodules["bernoulli"], submodules["poisson"]
    rng = np.random.default_rng(5)
    xc, xk, y = rng.uniform(-3, 3, (20, 2)), rng.integers(0, 2, (20, 1)), rng.integers(0, 2, 20)

    def fitted(sub=bern, **kw):
        flat, g = _hand_forest()
        m = module.LearnModel(SubModel=sub, **{**_HAND, **kw})
        m.set_hn_params(hn_metatree_list=nodes_from_flat(module, flat, g, sub.LearnModel))
        return widen_lcm(m)

    def cat_too_large():
        bad = xk.copy()
        bad[3, 0] = 3
        fitted().update_posterior(xc, bad, y, alg_type="given_MT")

    def nan_in_x():
        bad = xc.copy()
        bad[2, 0] = np.nan
        fitted().update_posterior(bad, xk, y, alg_type="given_MT")

    return {
        "wrong_shape_x_continuous": lambda: fitted().update_posterior(xc[:, :1], xk, y, alg_type="given_MT"),
        "wrong_shape_y": lambda: fitted().update_posterior(xc, xk, y[:5], alg_type="given_MT"),
        "wrong_rows_x_categorical": lambda: fitted().update_posterior(xc, xk[:5], y, alg_type="given_MT"),
        "categorical_value_too_large": cat_too_large,
        "squared_on_classifier": lambda: fitted().calc_pred_dist(xc, xk).make_prediction(loss="squared"),
        "pred_var_on_poisson": lambda: fitted(pois).calc_pred_dist(xc, xk).calc_pred_var(),
        "given_MT_without_forest": lambda: module.LearnModel(SubModel=bern, **_HAND).update_posterior(xc, xk, y,
                                                                                                     alg_type="given_MT"),
        "MTRF_with_three_children": lambda: module.LearnModel(SubModel=bern, **_HAND).update_posterior(xc, xk, y,
                                                                                                      alg_type="MTRF"),
        "nan_in_x_continuous": nan_in_x,
        "predict_categorical_value_too_large": lambda: fitted().predict(xc, np.where(xk == 1, 3, xk)),
        "predict_negative_categorical_value": lambda: fitted().predict(xc, -xk),
        "y_not_01": lambda: fitted().update_posterior(xc, xk, y + 1, alg_type="given_MT"),
        "float_x_categorical": lambda: fitted().update_posterior(xc, xk.astype(float), y, alg_type="given_MT"),
    }
