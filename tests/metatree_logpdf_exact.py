"""The predictive log-density of labelled rows under a meta-tree forest (include/mtpred.h), TEST INFRASTRUCTURE ONLY:
one evaluator of the definition over ``metatree_oracle.route`` paths and an engine's ``get_state()``, run with two
arithmetics.  ``MP`` is mpmath at 50 digits: the exact reference.  ``F64`` is binary64 NumPy: the same formulas in the
same order as the device, whose deviation from ``MP`` is the error the formulas themselves have in binary64.

``logpdf`` also returns M_i, the largest magnitude among the log-terms that entered row i (every lgamma, constant, product,
ln p_v, mixture operand and ln prob_b + value_b), so that a bound reads |lnp_i - exact_i| <= C eps (1 + M_i).
"""
import math
from types import SimpleNamespace

import mpmath as mp
import numpy as np
from scipy.special import gammaln

import metatree_oracle as orc

EPS = np.finfo(float).eps
BERNOULLI, CATEGORICAL, POISSON, EXPONENTIAL, NORMAL, LINREG = range(6)
WAVES = 4                                # include/mtpred.h: wave w mixes trees w, w + 4, ...
np.seterr(divide="ignore", over="ignore", invalid="ignore")          # ln 0 = -inf is part of the definition
F64 = SimpleNamespace(num=np.float64, log=np.log, log1p=np.log1p, exp=np.exp, lgamma=gammaln, sqrt=np.sqrt, pi=np.float64(math.pi))
MP = SimpleNamespace(num=mp.mpf, log=lambda v: mp.log(v) if v != 0 else mp.mpf("-inf"), log1p=mp.log1p, exp=mp.exp,
                     lgamma=mp.loggamma, sqrt=mp.sqrt, pi=mp.pi)


def node_consts(be, fam, D, post):
    """A node's constants as include/mtpred.h lists them, and the magnitudes of the log-terms inside them."""
    p = [be.num(float(v)) for v in post]
    if fam == BERNOULLI:
        s = p[0] + p[1]
        return [be.log(p[0] / s), be.log(p[1] / s)], []
    if fam == CATEGORICAL:
        s = sum(p[1:D], p[0])
        return [be.log(a / s) for a in p[:D]], []
    if fam == POISSON:
        c = [be.lgamma(p[0]), p[0] * be.log(p[1] / (1 + p[1])), be.log1p(p[1]), p[0]]
        return c, c[:2]
    if fam == EXPONENTIAL:
        return [be.log(p[0]) + p[0] * be.log(p[1]), p[0] + 1, p[1]], [be.log(p[0]), p[0] * be.log(p[1])]
    if fam == NORMAL:
        nu, lam = 2 * p[2], p[1] / (p[1] + 1) * p[2] / p[3]
        h, lg = (nu + 1) / 2, be.log(lam / nu)
        return [p[0], lam / nu, h, be.lgamma(h) - be.lgamma(nu / 2) + (lg - be.log(be.pi)) / 2], [be.lgamma(h), be.lgamma(nu / 2), lg]
    T = D * (D + 1) // 2
    lam = [[be.num(0)] * D for _ in range(D)]
    for k, (i, j) in enumerate(zip(*np.triu_indices(D))):
        lam[i][j] = p[D + k]
    U = [[be.num(0)] * D for _ in range(D)]                 # Lambda = U'U, in lr_cholesky's order
    for i in range(D):
        d = lam[i][i]
        for k in range(i):
            d -= U[k][i] * U[k][i]
        U[i][i] = be.sqrt(d)
        for j in range(i + 1, D):
            s = lam[i][j]
            for k in range(i):
                s -= U[k][i] * U[k][j]
            U[i][j] = s / U[i][i]
    W = [[be.num(0)] * D for _ in range(D)]                 # W = (U')^-1 by forward substitution, column by column
    for j in range(D):
        for i in range(j, D):
            t = be.num(1 if i == j else 0)
            for k in range(j, i):
                t -= U[k][i] * W[k][j]
            W[i][j] = t / U[i][i]
    ab, nu = p[D + T] / p[D + T + 1], 2 * p[D + T]
    h, lg = (nu + 1) / 2, be.log(ab / nu)
    return ([p[:D], W, ab / nu, h, be.lgamma(h) - be.lgamma(nu / 2) + (lg - be.log(be.pi)) / 2],
            [be.lgamma(h), be.lgamma(nu / 2), lg])


def node_logp(be, fam, D, c, x, y, lg1, mags):
    """ln p_v(y | x) from the node's constants; the magnitudes of its terms are appended to ``mags``."""
    ninf = be.num("-inf") if be is MP else be.num(-np.inf)
    if fam == BERNOULLI:
        return c[0] if y == 1 else c[1] if y == 0 else ninf
    if fam == CATEGORICAL:
        return c[int(y)] if 0 <= y < D else ninf
    if fam == POISSON:
        if y < 0:
            return ninf
        yd = be.num(int(y))
        terms = [be.lgamma(yd + c[3]), lg1, yd * c[2]]
        mags += terms
        return ((terms[0] - lg1) - c[0]) + (c[1] - terms[2])
    if fam == EXPONENTIAL:
        if y < 0:
            return ninf
        t = c[1] * be.log(c[2] + be.num(float(y)))
        mags.append(t)
        return c[0] - t
    if fam == NORMAL:
        r = be.num(float(y)) - c[0]
        t = c[2] * be.log1p(c[1] * (r * r))
        mags.append(t)
        return c[3] - t
    mu, W, s0, s1, s2 = c
    xs = [be.num(float(v)) for v in x[:D]]
    mean, q = be.num(0), be.num(0)
    for j in range(D):
        mean += xs[j] * mu[j]
    for a in range(D):
        u = be.num(0)
        for k in range(a + 1):
            u += W[a][k] * xs[k]
        q += u * u
    r = be.num(float(y)) - mean
    t1, t2 = be.log1p(q) / 2, s1 * be.log1p(s0 / (1 + q) * (r * r))
    mags += [t1, t2]
    return (s2 - t1) - t2


def logpdf(be, flat, state, fam, D, dim_cont, xc, xk, y):
    """(lnp [n] in the arithmetic ``be``, M [n] float): the definition, evaluated in the device's order."""
    paths = orc.route(flat, dim_cont, None if xc is None else np.asarray(xc, dtype=np.float64), xk)
    B, n, _ = paths.shape
    ninf = be.num("-inf") if be is MP else be.num(-np.inf)
    cache, out, M = {}, [], np.zeros(n)
    for i in range(n):
        mags = []
        lg1 = be.lgamma(be.num(int(y[i])) + 1) if fam == POISSON and y[i] >= 0 else None
        part = []
        for w in range(WAVES):
            mx, s = ninf, be.num(0)
            for b in range(w, B, WAVES):
                pb = be.num(float(state["prob"][b]))
                if not pb > 0:
                    continue
                walk = [int(v) for v in paths[b, i] if v >= 0]
                val = None
                for v in reversed(walk):
                    if v not in cache:
                        cache[v] = node_consts(be, fam, D, state["post"][v])
                    own = node_logp(be, fam, D, cache[v][0], None if xc is None else xc[i], y[i], lg1, mags)
                    mags += cache[v][1] + [own]
                    g = be.num(float(state["g"][v]))
                    if val is None or not g > 0:
                        val = own
                    elif g < 1:
                        a, c = be.log1p(-g) + own, be.log(g) + val
                        mags += [a, c]
                        val = max(a, c) if max(a, c) == ninf else max(a, c) + be.log1p(be.exp(-abs(a - c)))
                lt = be.log(pb) + val
                mags.append(lt)
                if lt > mx:
                    mx, s = lt, s * be.exp(mx - lt) + 1
                elif lt != ninf:
                    s += be.exp(lt - mx)
            part.append((mx, s))
        top = max(m for m, _ in part)
        out.append(top if top == ninf else top + be.log(sum((s * be.exp(m - top) for m, s in part if m != ninf), be.num(0))))
        M[i] = max([abs(float(t)) for t in mags if t is not None and math.isfinite(float(t))], default=0.0)
    return out, M


def ratios(got, exact, M):
    """err_i / (eps (1 + M_i)) of binary64 values ``got`` against mpmath values ``exact``; -inf must sit where -inf does."""
    r = np.zeros(len(got))
    for i, (u, e) in enumerate(zip(got, exact)):
        if e == mp.mpf("-inf") or u == -np.inf:
            r[i] = 0.0 if (e == mp.mpf("-inf") and u == -np.inf) else np.inf
        else:
            r[i] = float(abs(mp.mpf(float(u)) - e)) / (EPS * (1.0 + M[i]))
    return r


# ---- the cases both test files share ----------------------------------------------------------------------------------------
def posts(fam, D, nodes, rng, alpha=(1.0, 10.0)):
    """Plausible posterior vectors [nodes, n_post] of a family (include/mtree.h, mtree_stat_cols)."""
    u = lambda lo, hi, *s: rng.uniform(lo, hi, size=(nodes, *s))          # noqa: E731
    if fam == LINREG:
        x = rng.standard_normal((nodes, 2 * D, D))
        lam = np.eye(D) + x.transpose(0, 2, 1) @ x
        return np.concatenate([rng.standard_normal((nodes, D)), lam[(slice(None), *np.triu_indices(D))], u(*alpha, 1), u(1, 10, 1),
                               np.full((nodes, 1), 9.0)], axis=1)
    return {BERNOULLI: lambda: u(0.5, 20, 2), CATEGORICAL: lambda: u(0.5, 10, D), POISSON: lambda: u(1, 10, 3),
            EXPONENTIAL: lambda: u(1, 10, 2),
            NORMAL: lambda: np.concatenate([2 * rng.standard_normal((nodes, 1)), u(1, 10, 1), u(*alpha, 1), u(1, 10, 2)], axis=1)}[fam]()


def labels(fam, D, n, rng):
    return {BERNOULLI: lambda: rng.integers(0, 2, n), CATEGORICAL: lambda: rng.integers(0, D, n), POISSON: lambda: rng.poisson(4.0, n),
            EXPONENTIAL: lambda: rng.exponential(2.0, n)}.get(fam, lambda: 3.0 * rng.standard_normal(n))()


def make(fam, specs, xc, xk, cat_card, seed, D=None, alpha=(1.0, 10.0)):
    """A forest of ``metatree_lr_cases.forest`` specs with random posteriors, g in (0.05, 0.95) and Dirichlet weights."""
    import metatree_lr_cases as lc
    rng = np.random.default_rng(seed)
    flat = lc.forest(specs)
    nodes, B = len(flat["feat"]), len(specs)
    D = D if D is not None else (3 if fam == CATEGORICAL else xc.shape[1] if fam == LINREG else 0)
    state = dict(g=rng.uniform(0.05, 0.95, nodes), post=posts(fam, D, nodes, rng, alpha), lml=np.zeros(nodes), lcm=np.zeros(nodes),
                 prob=rng.dirichlet(np.ones(B)))
    n = len(xc if xc is not None else xk)
    return dict(fam=fam, D=D, flat=flat, state=state, dim_cont=0 if xc is None else xc.shape[1], dim_cat=0 if xk is None else xk.shape[1],
                cat_card=np.array(cat_card, np.int32), xc=xc, xk=xk, y=labels(fam, D, n, rng))


def grid_case(fam, n, B, depth, dtype=np.float64, dim_cont=None):
    """Test 1's forest: root-only trees (depth 0), or five shapes of unequal depth up to 3 over x0, x1 and one three-way
    categorical feature; at depth 3 every seventh row cannot be routed (NaN x0; for linear regression, whose x0 is a
    regressor, a categorical value no node has) and stops at an inner node."""
    import metatree_lr_cases as lc
    dc = dim_cont or (3 if fam == LINREG else 2)
    rng = np.random.default_rng(1000 * fam + 10 * n + B)
    xc, xk = rng.uniform(-4, 4, (n, dc)).astype(dtype), rng.integers(0, 3, (n, 1))
    shapes = [lc.full_binary(3), None, (dc, None, [lc.STUMP, None, (0, [1.0], [None, (dc, None, [None, None, None])])]), lc.STUMP,
              (1, [-1.0, 1.0], [None, lc.full_binary(2), None])]
    if depth:
        if fam == LINREG:
            xk[::7] = 7
        else:
            xc[::7, 0] = np.nan
    return make(fam, [shapes[b % 5] if depth else None for b in range(B)], xc, xk, [3], seed=n + B)


def paths_case(D, share):
    """Linear regression under a sixteen-way categorical root over four-way splits of x0.  Tile 0: the children hold
    share - 1, share and at most three lanes; tile 1: all 64 lanes in one child; tile 2: 64 distinct stop nodes."""
    child = np.concatenate([np.repeat([0, 1], [share - 1, share]), 2 + np.arange(64 - 2 * share + 1) % 14, np.full(64, 5),
                            np.arange(64) // 4])
    rng = np.random.default_rng(D)
    xc = rng.uniform(-2, 2, (192, D))
    xc[:, 0] = np.concatenate([rng.uniform(-2, 2, 128), -1.5 + np.arange(64) % 4])
    four = (0, [-1.0, 0.0, 1.0], [None] * 4)
    return make(LINREG, [(D, None, [four] * 16)], xc, child[:, None].astype(np.int64), [16], seed=60 + D)


# the worst |F64 - MP| / (eps (1 + M)) of ``evaluate`` over GRID x the six families and paths_case(1 | 4 | 15), measured once
# on the CPU, and the device's allowance: 4 x that, for fused multiply-adds and the MFMA's order of sums
MEASURED = 1.388
C = 4 * MEASURED
GRID = [(1, 1, 0, np.float64), (63, 3, 3, np.float32), (64, 4, 3, np.float64), (65, 5, 0, np.float32), (257, 9, 3, np.float64)]


def evaluate(case, be):
    return logpdf(be, case["flat"], case["state"], case["fam"], case["D"], case["dim_cont"], case["xc"], case["xk"], case["y"])
