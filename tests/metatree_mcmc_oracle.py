"""NumPy restatement of metatree's MTMCMC / REMTMCMC (TEST INFRASTRUCTURE ONLY): the proposal, the two chains and the merge of
equal trees, with a pluggable draw provider.

Semantics are the reference's (bayesml/metatree/_metatree.py:2036-2665), on capacity tables instead of ``_Node`` trees: a
chain's tree is a complete C-ary tree of ``cap`` slots in heap order (children of h: C h + 1 .. C h + C) with per slot
``feat`` (-1 for a leaf or a slot no row reaches), ``thr[cap, C + 1]``, ``g``, ``post[cap, P]``, ``lml``, ``cnt``, ``first``
(lowest row index) and ``dflag`` (0 not visited by the keep / flip test, 1 kept, 2 flipped); ``node[n]`` is the slot where each
row stops.  The walk is depth-first, children left to right, exactly the order in which the reference consumes its stream.

Draw providers:
  ``Stream(rng)``      consumes ``np.random.default_rng(seed)`` as the reference does: the discarded root draw of every fresh
                       ``_Node`` (:2081, :2443, :2500), ``rng.choice`` of a list for a feature, ``rng.random()`` for the keep /
                       flip, acceptance and exchange tests, ``rng.choice(B - 1)`` for the exchanged pair.
  ``Addressed(seed)``  the engine's addressed tables: step t, chain b, slot h uses
                       ``node_table(seed, t, B, cap)[b, h]``; acceptance and exchange draws come from ``aux_table``.
"""
import numpy as np

import metatree_lr_oracle as lro
import metatree_oracle as mo

LINREG = 5


# ---- the addressed tables -----------------------------------------------------------------------------------------------------
def node_table(seed, t, B, cap):
    """[B, cap, 2]: (keep / flip draw, feature draw) of every slot at step t.  The step sits in the THIRD counter word: Philox
    counts its blocks in the first, so tables at consecutive first words would overlap."""
    return np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, t, 0])).random((B, cap, 2))


def aux_table(seed, t, B, num_exchange=0):
    """[B + 2 num_exchange]: the chains' acceptance draws of step t, then (pair draw, test draw) of every exchange."""
    return np.random.Generator(np.random.Philox(key=seed, counter=[0, 0, t, 1])).random(B + 2 * num_exchange)


def capacity(C, depth):
    return (C ** (depth + 1) - 1) // (C - 1)


class TableDraws:
    """Addressed draws of one step from explicit tables."""

    def __init__(self, nodes, aux=None, B=1):
        self.nodes, self.aux, self.B = nodes, aux, B

    def new_root(self, b, F):
        pass

    def keep(self, b, h):
        return self.nodes[b, h, 0]

    def feature(self, b, h, F):
        return min(F - 1, int(np.floor(self.nodes[b, h, 1] * F)))

    def other(self, b, h, F, last_k):
        k = min(F - 2, int(np.floor(self.nodes[b, h, 1] * (F - 1))))
        return k + 1 if k >= last_k else k

    def accept(self, b):
        return self.aux[b]

    def exchange(self, e, B):
        return min(B - 2, int(np.floor(self.aux[self.B + 2 * e] * (B - 1)))), self.aux[self.B + 2 * e + 1]


class Addressed:
    def __init__(self, seed, B, cap, num_exchange=0):
        self.seed, self.B, self.cap, self.num_exchange = seed, B, cap, num_exchange

    def at(self, t):
        return TableDraws(node_table(self.seed, t, self.B, self.cap), aux_table(self.seed, t, self.B, self.num_exchange),
                          self.B)


class Stream:
    """The reference's single PCG64 stream."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def at(self, t):
        return self

    def new_root(self, b, F):
        self.rng.choice(list(range(F)))

    def keep(self, b, h):
        return self.rng.random()

    def feature(self, b, h, F):
        return int(self.rng.choice(list(range(F))))

    def other(self, b, h, F, last_k):
        return int(self.rng.choice([k for k in range(F) if k != last_k]))

    def accept(self, b):
        return self.rng.random()

    def exchange(self, e, B):
        j = int(self.rng.choice(B - 1))
        return j, self.rng.random()


# ---- the configuration and the tables ----------------------------------------------------------------------------------------
class Config:
    def __init__(self, fam, degree, dim_cont, dim_cat, C, max_depth, h0, sub_hn, g_root, g_below, threshold_type):
        self.fam, self.degree, self.dc, self.dk, self.C, self.max_depth = fam, degree, dim_cont, dim_cat, C, max_depth
        self.h0, self.sub_hn = np.asarray(h0, dtype=float), np.asarray(sub_hn, dtype=float)
        self.g_root, self.g_below, self.threshold_type = g_root, g_below, threshold_type
        self.F = dim_cont + dim_cat
        self.cap = capacity(C, max_depth)
        self.depth = np.zeros(self.cap, dtype=np.int64)
        for h in range(1, self.cap):
            self.depth[h] = self.depth[(h - 1) // C] + 1


def new_tables(cfg, n):
    g = np.where(cfg.depth == cfg.max_depth, 0.0, cfg.g_below)
    g[0] = cfg.g_root
    return dict(feat=np.full(cfg.cap, -1, dtype=np.int64), thr=np.zeros((cfg.cap, cfg.C + 1)), g=g,
                post=np.tile(cfg.sub_hn, (cfg.cap, 1)), lml=np.full(cfg.cap, np.nan), lcm=np.zeros(cfg.cap), cnt=np.zeros(cfg.cap, dtype=np.int64),
                first=np.full(cfg.cap, -1, dtype=np.int64), dflag=np.zeros(cfg.cap, dtype=np.int64),
                node=np.zeros(n, dtype=np.int64), L=np.nan)


def make_thresholds(x):
    """ref:54-80, as it stands; also returns (best metric, second-best metric) for the fixtures' margins."""
    u = np.unique(x)
    th, n_l, s_l, q_l = 0, 1, u[0], u[0] * u[0]
    n_r, s_r, q_r = len(u) - 1, u[1:].sum(), (u[1:] * u[1:]).sum()
    best = (q_l - s_l * s_l / n_l) + (q_r - s_r * s_r / n_r)
    metrics = [best]
    for i in range(1, len(u) - 1):
        n_l += 1
        s_l += u[i]
        q_l += u[i] * u[i]
        n_r -= 1
        s_r -= u[i]
        q_r -= u[i] * u[i]
        metric = (q_l - s_l * s_l / n_l) + (q_r - s_r * s_r / n_r)
        metrics.append(metric)
        if metric < best:
            best, th = metric, i
    return np.array([u.min(), (u[th] + u[th + 1]) / 2, u.max()]), np.sort(metrics)[:2]


def thresholds(cfg, x, margins=None):
    """ref:2636-2650 for a continuous split on the node's values x."""
    lo, hi = x.min(), x.max()
    if lo == hi:
        return np.ones(cfg.C + 1) * lo
    if cfg.threshold_type == "1d_kmeans" and cfg.C == 2:
        t, two = make_thresholds(x)
        if margins is not None and len(two) == 2:
            margins.append(abs(two[1] - two[0]) / max(abs(two[1]), abs(two[0]), 1e-300))
        return t
    return np.arange(lo, hi + (hi - lo) / cfg.C / 2, (hi - lo) / cfg.C)


def child_masks(cfg, k, t, xc, xk):
    """The reference's masks of the C children (ref:2391-2417) on the node's own rows."""
    C = cfg.C
    if k < cfg.dc:
        x = xc[:, k]
        with np.errstate(invalid="ignore"):
            return [x < t[1] if i == 0 else t[i] <= x if i == C - 1 else (t[i] <= x) & (x < t[i + 1]) for i in range(C)]
    return [xk[:, k - cfg.dc] == i for i in range(C)]


def fold(cfg, X, y):
    """(post vector, lml) of a node's rows from sub_hn, in plain float64 as the scalar learners compute it."""
    if cfg.fam == LINREG:
        D = cfg.degree
        mu0, lam0, alpha, beta, n = lro.unpack(cfg.sub_hn, D)
        x = np.asarray(X, dtype=float)[:, :D]
        lam = lam0 + x.T @ x
        mu = np.linalg.solve(lam, x.T @ y + lam0 @ mu0)
        p = lro.pack(mu, lam, alpha + len(y) / 2.0, beta + (-mu @ lam @ mu + y @ y + mu0 @ lam0 @ mu0) / 2.0, n + len(y))
        return p, lro.lml_plain(cfg.h0, p, D)
    p = mo._plain_fold(cfg.fam, cfg.degree, cfg.sub_hn, y)
    return p, mo._plain_lml(cfg.fam, cfg.h0, p, p[4] if cfg.fam == mo.NORMAL else p[2] if cfg.fam == mo.POISSON else 0.0)


# ---- one proposal ---------------------------------------------------------------------------------------------------------
def grow(cfg, xc, xk, y, draws, b, last, g_max, margins=None, levels=None, fresh_root=True):
    """``_generate_truncated_and_update`` from the root (``last`` None: the initial tree, every node regenerated).  ``levels``
    stops the growth after that many levels (the nodes below stay unopened), for the one-level kernel tests."""
    n = len(y)
    T = new_tables(cfg, n)
    xc = np.zeros((n, 0)) if xc is None else np.asarray(xc, dtype=np.float64)
    xk = np.zeros((n, 0), dtype=np.int64) if xk is None else np.asarray(xk).astype(np.int64)
    C, F = cfg.C, cfg.F
    if margins is None:
        margins = []

    def rec(h, rows, regen):
        d = int(cfg.depth[h])
        T["cnt"][h], T["first"][h] = len(rows), rows[0]
        T["post"][h], T["lml"][h] = fold(cfg, xc[rows], y[rows])
        lml = T["lml"][h]
        T["node"][rows] = h
        if d == cfg.max_depth or (np.allclose(xc[rows], xc[rows[0]]) and np.allclose(xk[rows], xk[rows[0]])):
            T["g"][h] = 0.0
            return lml
        if levels is not None and d >= levels:
            return lml
        if regen:
            k = draws.feature(b, h, F)
        else:
            u, bound = draws.keep(b, h), min(last["g"][h], g_max)
            margins.append(abs(u - bound) / max(u, bound, 1e-300))
            if u > bound:
                regen = True
                T["dflag"][h] = 2
                k = draws.other(b, h, F, int(last["feat"][h]))
            else:
                T["dflag"][h] = 1
                k = int(last["feat"][h])
        T["feat"][h] = k
        t = None
        if k < cfg.dc:
            t = thresholds(cfg, xc[rows, k], margins)
            T["thr"][h, :len(t)] = t
        Ls = []
        for i, m in enumerate(child_masks(cfg, k, t, xc[rows], xk[rows])):
            Ls.append(rec(C * h + 1 + i, rows[m], regen) if m.any() else 0.0)
            T["lcm"][C * h + 1 + i] = Ls[-1]
        g0 = T["g"][h]
        with np.errstate(divide="ignore"):
            t1 = np.log(g0) + np.array(Ls).sum()
            L = np.logaddexp(np.log(1 - g0) + lml, t1)
        T["g"][h] = np.exp(t1 - L)
        return L

    if fresh_root:
        draws.new_root(b, F)
    T["L"] = float(rec(0, np.arange(n), last is None))
    return T


def truncated_posterior(cfg, T, dflag, g_max):
    """``_calc_truncated_posterior_lean`` (ref:2612-2621) with the division flags of the last proposal."""
    def rec(h):
        if dflag[h] == 0:
            return 0.0
        with np.errstate(divide="ignore"):
            if dflag[h] == 2:
                return np.log(1.0 - min(T["g"][h], g_max))
            tmp = 0
            for i in range(cfg.C):
                tmp += rec(cfg.C * h + 1 + i)
            return np.log(min(T["g"][h], g_max)) + tmp
    return rec(0)


def same_tree(cfg, a, b, h=0):
    """ref:1819-1843 on capacity tables."""
    if a["feat"][h] < 0 or b["feat"][h] < 0:
        return bool(a["feat"][h] < 0 and b["feat"][h] < 0)
    if a["feat"][h] != b["feat"][h]:
        return False
    if a["feat"][h] < cfg.dc and not np.allclose(a["thr"][h], b["thr"][h]):
        return False
    return all(same_tree(cfg, a, b, cfg.C * h + 1 + i) for i in range(cfg.C))


def merge(cfg, trees, prob):
    trees, prob = list(trees), np.array(prob, dtype=float)
    for i in range(len(trees)):
        for j in range(i + 1, len(trees)):
            if same_tree(cfg, trees[i], trees[j]):
                trees[i] = None
                prob[j] += prob[i]
                prob[i] = -1
                break
    return [t for t in trees if t is not None], prob[prob > -0.5]


# ---- the chains -----------------------------------------------------------------------------------------------------------
def mtmcmc(cfg, xc, xk, y, provider, burn_in=100, num_metatrees=500, g_max=0.0, rho=0.99, phi=0.999, p_obj=0.3):
    """ref:2096-2133.  Returns the trace and the merged (trees, prob)."""
    tr = dict(l_new=[], tp_new=[], tp_last=[], accept=[], g_max=[], margins=[])
    trees, counts = [grow(cfg, xc, xk, y, provider.at(0), 0, None, g_max, tr["margins"])], [1]
    l_last = trees[0]["L"]
    if cfg.F == 1:
        return tr, trees, np.array([1.0])
    proposed = accepted = 1
    numer = denom = 0.0
    gm_acc = gm_den = 0.0

    def step():
        nonlocal l_last, proposed, accepted, numer, denom
        draws = provider.at(proposed)
        new = grow(cfg, xc, xk, y, draws, 0, trees[-1], g_max, tr["margins"])
        tp_new = truncated_posterior(cfg, new, new["dflag"], g_max)
        tp_last = truncated_posterior(cfg, trees[-1], new["dflag"], g_max)
        u, a = draws.accept(0), np.exp(new["L"] - tp_last - l_last + tp_new)
        tr["margins"].append(abs(u - a) / max(u, a, 1e-300))
        ok = u < a
        for key, val in (("l_new", new["L"]), ("tp_new", tp_new), ("tp_last", tp_last), ("accept", ok)):
            tr[key].append(val)
        numer *= rho
        denom = denom * rho + 1
        if ok:
            trees.append(new)
            counts.append(1)
            l_last = new["L"]
            accepted += 1
            numer += 1
        else:
            counts[-1] += 1
        proposed += 1

    while proposed < burn_in:
        step()
        p_hat = numer / denom
        g_new = g_max * p_obj / p_hat if p_hat > p_obj else 1.0 - (1.0 - g_max) * (1.0 - p_obj) / (1.0 - p_hat)
        gm_acc = gm_acc * phi + g_new
        gm_den = gm_den * phi + 1
        g_max = gm_acc / gm_den
        tr["g_max"].append(g_max)
    tmp = accepted - 1
    counts[-1] = 1
    while proposed < burn_in + num_metatrees:
        step()
    prob = np.array(counts[tmp:], dtype=float)
    return (tr,) + merge(cfg, trees[tmp:], prob / prob.sum())


def remtmcmc(cfg, xc, xk, y, provider, burn_in=100, num_metatrees=500, num_chains=8, g_max=0.9, beta_vec=None,
             num_interval=10, num_exchange=4):
    """ref:2211-2256."""
    B = num_chains
    tr = dict(l_new=[], tp_new=[], tp_last=[], accept=[], exchange=[], l_list=[], margins=[])
    d0 = provider.at(0)
    for b in range(B):          # the reference makes every chain's root (one discarded draw each) before it grows the first
        d0.new_root(b, cfg.F)
    lists = [[grow(cfg, xc, xk, y, d0, b, None, g_max, tr["margins"], fresh_root=False)] for b in range(B)]
    counts = [[1] for _ in range(B)]
    l_lasts = np.array([lists[b][0]["L"] for b in range(B)])
    if cfg.F == 1:
        return tr, lists[B - 1], np.array([1.0])
    beta = (np.arange(B) + 1) / B
    if beta_vec is not None:
        beta[:] = beta_vec
    t = 0

    def step():
        nonlocal t
        t += 1
        draws = provider.at(t)
        row = dict(l_new=[], tp_new=[], tp_last=[], accept=[])
        for b in range(B):
            new = grow(cfg, xc, xk, y, draws, b, lists[b][-1], g_max, tr["margins"])
            tp_new = truncated_posterior(cfg, new, new["dflag"], g_max)
            tp_last = truncated_posterior(cfg, lists[b][-1], new["dflag"], g_max)
            u, a = draws.accept(b), np.exp((new["L"] - l_lasts[b]) * beta[b] - tp_last + tp_new)
            tr["margins"].append(abs(u - a) / max(u, a, 1e-300))
            ok = u < a
            for key, val in (("l_new", new["L"]), ("tp_new", tp_new), ("tp_last", tp_last), ("accept", ok)):
                row[key].append(val)
            if ok and b == B - 1:
                lists[b].append(new)
                counts[b].append(1)
                l_lasts[b] = new["L"]
            elif ok:
                lists[b][-1] = new
                counts[b][-1] = 1
                l_lasts[b] = new["L"]
            else:
                counts[b][-1] += 1
        for key, val in row.items():
            tr[key].append(val)
        tr["l_list"].append(l_lasts[-1])
        return draws

    def exchange(draws):
        tr["exchange"].append(-1)
        for e in range(num_exchange):
            j, u = draws.exchange(e, B)
            a = np.exp(l_lasts[j] * beta[j + 1] + l_lasts[j + 1] * beta[j] - l_lasts[j] * beta[j] - l_lasts[j + 1] * beta[j + 1])
            tr["margins"].append(abs(u - a) / max(u, a, 1e-300))
            if not u < a:
                continue
            tr["exchange"].append(j)
            if j == B - 2:
                lists[j + 1].append(lists[j][-1])
                lists[j][-1] = lists[j + 1][-2]
                counts[j][-1] = 1
                counts[j + 1][-1] -= 1
                counts[j + 1].append(1)
                l_lasts[j], l_lasts[j + 1] = l_lasts[j + 1], l_lasts[j]
                tr["l_list"].append(l_lasts[j + 1])
            else:
                lists[j + 1][-1], lists[j][-1] = lists[j][-1], lists[j + 1][-1]
                counts[j][-1] = counts[j + 1][-1] = 1
                l_lasts[j], l_lasts[j + 1] = l_lasts[j + 1], l_lasts[j]

    for i in range(burn_in):
        draws = step()
        if B > 1 and i % num_interval == 0:
            exchange(draws)
    tmp = len(counts[B - 1]) - 1
    for b in range(B):
        counts[b][-1] = 1
    for i in range(num_metatrees):
        draws = step()
        if B > 1 and i % num_interval == 0:
            exchange(draws)
    prob = np.array(counts[B - 1][tmp:], dtype=float)
    return (tr,) + merge(cfg, lists[B - 1][tmp:], prob / prob.sum())


# ---- the golden cases (tests/golden/make_golden_metatree_mcmc.py writes them from the reference) ---------------------------
FAMILY = dict(bernoulli=mo.BERNOULLI, normal=mo.NORMAL, linearregression=LINREG)
CASES = [
    dict(name="mtmcmc_bern_kmeans_d3", alg="MTMCMC", sub="bernoulli", C=2, depth=3, dc=2, dk=1, n=300, threshold="1d_kmeans",
         kw=dict(burn_in=20, num_metatrees=30)),
    dict(name="mtmcmc_normal_mid_c3_d2", alg="MTMCMC", sub="normal", C=3, depth=2, dc=2, dk=1, n=250, threshold="sample_midpoint",
         kw=dict(burn_in=15, num_metatrees=25)),
    dict(name="mtmcmc_linreg_kmeans_d2", alg="MTMCMC", sub="linearregression", C=2, depth=2, dc=2, dk=1, n=200,
         threshold="1d_kmeans", kw=dict(burn_in=12, num_metatrees=20)),
    dict(name="mtmcmc_bern_mid_d1", alg="MTMCMC", sub="bernoulli", C=2, depth=1, dc=3, dk=0, n=120, threshold="sample_midpoint",
         kw=dict(burn_in=10, num_metatrees=20)),
    dict(name="remtmcmc_1_bern_kmeans_d2", alg="REMTMCMC", sub="bernoulli", C=2, depth=2, dc=2, dk=1, n=200, threshold="1d_kmeans",
         kw=dict(burn_in=10, num_metatrees=20, num_chains=1)),
    dict(name="remtmcmc_2_normal_kmeans_d2", alg="REMTMCMC", sub="normal", C=2, depth=2, dc=2, dk=1, n=200, threshold="1d_kmeans",
         kw=dict(burn_in=10, num_metatrees=20, num_chains=2, num_interval=3)),
    dict(name="remtmcmc_8_bern_kmeans_d3", alg="REMTMCMC", sub="bernoulli", C=2, depth=3, dc=2, dk=1, n=300, threshold="1d_kmeans",
         kw=dict(burn_in=12, num_metatrees=30, num_chains=8, num_interval=4)),
    dict(name="remtmcmc_8_linreg_mid_c3_d2", alg="REMTMCMC", sub="linearregression", C=3, depth=2, dc=2, dk=1, n=240,
         threshold="sample_midpoint", kw=dict(burn_in=8, num_metatrees=16, num_chains=8, num_interval=2, num_exchange=3)),
]
TRACE = ("l_new", "tp_new", "tp_last", "accept")


def case_inputs(case):
    """The seeded sample of a case: features rounded to three decimals (so unique values repeat), y planted on feature 1."""
    rng = np.random.default_rng(sum(case["name"].encode()))
    n, dc, dk, C = case["n"], case["dc"], case["dk"], case["C"]
    xc = np.round(rng.uniform(-1, 1, (n, dc)), 3)
    xk = rng.integers(0, C, (n, dk))
    left = xc[:, 1] < 0.1
    if case["sub"] == "bernoulli":
        y = (rng.random(n) < np.where(left, 0.15, 0.85)).astype(np.int64)
    elif case["sub"] == "normal":
        y = np.where(left, -1.0, 2.0) + 0.3 * rng.standard_normal(n)
    else:
        y = np.where(left, -1.0, 2.0) * xc[:, 0] + 0.5 * xc[:, 1] + 0.3 * rng.standard_normal(n)
    return dict(xc=xc, xk=xk, y=y)


def case_h0(case):
    return {"bernoulli": np.array([0.5, 0.5]), "normal": np.array([0.0, 1.0, 1.0, 1.0, 0.0]),
            "linearregression": lro.default_h0(case["dc"])}[case["sub"]]


def case_config(case):
    h0 = case_h0(case)
    degree = case["dc"] if case["sub"] == "linearregression" else 0
    return Config(FAMILY[case["sub"]], degree, case["dc"], case["dk"], case["C"], case["depth"], h0, h0, 0.5, 0.5,
                  case["threshold"])


def run_case(case, provider):
    """(trace, merged trees, prob) of a case's chain under a draw provider."""
    cfg, inp = case_config(case), case_inputs(case)
    xk = inp["xk"] if case["dk"] else None
    run = mtmcmc if case["alg"] == "MTMCMC" else remtmcmc
    return run(cfg, inp["xc"], xk, inp["y"], provider, **case["kw"])


def stack(cfg, trees):
    """The list as arrays [trees, cap, ...]: feat, thr, g, post."""
    return {k: np.array([t[k] for t in trees]) for k in ("feat", "thr", "g", "post")}
