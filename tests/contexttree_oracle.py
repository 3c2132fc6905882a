"""NumPy oracle of the context-tree engine (TEST INFRASTRUCTURE ONLY): the batch form of the reference's sequential
``update_posterior`` (DESIGN.md "Context tree") and its MAP sweep on dense per-level tables.

A table set is a dict of flat arrays over all levels, level d starting at ``offsets(k, D)[d]``, keys in order:
``g[nodes]``, ``beta[nodes, k]`` (float64), ``exists[nodes]``, ``leaf[nodes]`` (uint8).  The key of the context
``(x[i-1], ..., x[i-d])`` is ``sum_j x[i-j] k^(j-1)``; child c of key s at depth d is key ``s + c k^d``.
"""
import numpy as np
from scipy.special import gammaln


def offsets(k, D):
    off = [0]
    for d in range(D + 1):
        off.append(off[-1] + k ** d)
    return off


def new_tables(k, D):
    n = offsets(k, D)[-1]
    return dict(g=np.zeros(n), beta=np.zeros((n, k)), exists=np.zeros(n, np.uint8), leaf=np.zeros(n, np.uint8))


def copy_tables(t):
    return {name: a.copy() for name, a in t.items()}


def context_keys(x, k, D):
    """keys[d][i - d] = key of sample i at depth d, for i >= d."""
    x = np.asarray(x, dtype=np.int64)
    keys = [np.zeros(len(x), dtype=np.int64)]
    for d in range(1, D + 1):
        if len(x) < d:
            keys.append(np.zeros(0, dtype=np.int64))
            continue
        keys.append(keys[-1][1:] + x[:len(x) - d] * k ** (d - 1))
    return keys


def level_counts(x, k, D):
    """cnt[d][s, a] = number of samples that pass through (or end at) node s of level d with symbol a."""
    x = np.asarray(x, dtype=np.int64)
    keys = context_keys(x, k, D)
    cnt = []
    for d in range(D + 1):
        flat = keys[d] * k + x[d:] if len(x) > d else np.zeros(0, dtype=np.int64)
        cnt.append(np.bincount(flat, minlength=k ** (d + 1)).reshape(k ** d, k).astype(np.int64))
    return cnt


def deepest_counts(x, k, D):
    """What ctree_count returns: (bad, cnt_D) with every sample dropped that has a bad symbol in x[i-D..i]."""
    x = np.asarray(x, dtype=np.int64)
    ok = (x >= 0) & (x < k)
    xs = np.where(ok, x, 0)
    c = np.zeros((k ** D, k), dtype=np.int64)
    if len(x) > D:
        win = np.lib.stride_tricks.sliding_window_view(ok, D + 1).all(axis=1)
        keys = context_keys(xs, k, D)[D]
        np.add.at(c, (keys[win], xs[D:][win]), 1)
    return int((~ok).sum()), c


def logdm(b0, n):
    return gammaln(b0.sum(-1)) - gammaln((b0 + n).sum(-1)) + (gammaln(b0 + n) - gammaln(b0)).sum(-1)


def batch_update(x, k, D, t, hn_g, hn_beta_vec):
    """One ``update_posterior(x)`` on the tables ``t``, in place.  Returns the per-level counts."""
    x = np.asarray(x, dtype=np.int64)
    N, off = len(x), offsets(k, D)
    cnt = level_counts(x, k, D)
    keys = context_keys(x, k, D)
    hn_beta_vec = np.asarray(hn_beta_vec, dtype=float)
    logw = None
    for d in range(D, -1, -1):
        sl = slice(off[d], off[d + 1])
        ex = t["exists"][sl] != 0
        b0 = np.where(ex[:, None], t["beta"][sl], hn_beta_vec[None, :])
        g0 = np.where(ex, t["g"][sl], 0.0 if d == D else hn_g)
        n = cnt[d].astype(float)
        touched = cnt[d].sum(-1) > 0
        if d == D:
            w, newg = logdm(b0, n), g0
        else:
            S = logw.reshape(k, k ** d).sum(0)
            bp, lead = b0.copy(), np.zeros(k ** d)
            if N > d:
                kk = keys[d][0]
                lead[kk] = np.log(b0[kk, x[d]] / b0[kk].sum())
                bp[kk, x[d]] += 1
                n[kk, x[d]] -= 1
            with np.errstate(divide="ignore", invalid="ignore"):
                a = np.log1p(-g0) + logdm(bp, n)
                b = np.log(g0) + S
                mix = np.logaddexp(a, b)
                newg = np.where(g0 > 0, np.exp(b - mix), 0.0)
            w = lead + mix
        logw = np.where(touched, w, 0.0)
        t["beta"][sl] = np.where(touched[:, None], b0 + cnt[d], t["beta"][sl])
        t["g"][sl] = np.where(touched, newg, t["g"][sl])
        t["exists"][sl] = np.where(touched, 1, t["exists"][sl])
        if d == D:
            t["leaf"][sl] = np.where(touched & ~ex, 1, t["leaf"][sl])
    return cnt


# ---- the exact oracle: the same update in mpmath, for the tests that hold the kernels' floating-point formula to it ----------
MP_DPS = 60


def _mp():
    import mpmath
    mpmath.mp.dps = MP_DPS
    return mpmath


def _mp_row(b, n):
    mp = _mp()
    return [mp.mpf(float(v)) for v in b], [int(v) for v in n]


def logdm_exact(b, n):
    """lnDM(b, n) of one row (binary64 b taken as exact, integer n) as an mpf of MP_DPS digits."""
    mp = _mp()
    b, n = _mp_row(b, n)
    return (mp.loggamma(mp.fsum(b)) - mp.loggamma(mp.fsum(b) + sum(n))
            + mp.fsum(mp.loggamma(v + c) - mp.loggamma(v) for v, c in zip(b, n) if c != 0))


def row_scale(b, n):
    """The sizes of the terms lnDM adds: sum_a |lnG(b_a + n_a) - lnG(b_a)| + |lnG(sum b + sum n) - lnG(sum b)| (float)."""
    mp = _mp()
    b, n = _mp_row(b, n)
    s = mp.fsum(abs(mp.loggamma(v + c) - mp.loggamma(v)) for v, c in zip(b, n) if c != 0)
    return float(s + abs(mp.loggamma(mp.fsum(b) + sum(n)) - mp.loggamma(mp.fsum(b))))


def head_key(head, k, d):
    """Key at depth d of the head sample x[d] (its context is x[d-1], ..., x[0])."""
    return sum(int(head[d - j]) * k ** (j - 1) for j in range(1, d + 1))


def counts_from_deepest(cnt_deepest, head, k, D):
    """[cnt_0, ..., cnt_D] from the deepest level's table and the first min(N, D) symbols: child sums plus the head samples."""
    cnt = [None] * (D + 1)
    cnt[D] = np.asarray(cnt_deepest, dtype=np.int64).reshape(k ** D, k)
    for d in range(D - 1, -1, -1):
        cnt[d] = cnt[d + 1].reshape(k, k ** d, k).sum(0)
        if len(head) > d:
            cnt[d][head_key(head, k, d), int(head[d])] += 1
    return cnt


def batch_update_exact(cnt_deepest, head, k, D, t, hn_g, hn_beta_vec):
    """``batch_update`` in mpmath on the tables ``t`` (not modified), from the deepest level's count table and the head
    (the first min(N, D) symbols of the sample; ``sweep`` takes the same two).  Returns a dict over all nodes:
    ``g`` (object array of mpf: the exact new h_g; the old one where the node has no samples), ``B`` (float: the sum over
    the node's subtree of row_scale + |logit g0| + |lead| of the touched nodes - the sizes of the terms that enter the
    node's log-odds; logit g0 counts only for 0 < g0 < 1, where the logarithms are taken), ``beta``, ``exists`` (what the
    update leaves), ``touched`` and ``logit`` (the exact new log-odds where 0 < g0 < 1, else None)."""
    mp = _mp()
    off = offsets(k, D)
    head = [int(v) for v in head][:D]
    cnt = counts_from_deepest(cnt_deepest, head, k, D)
    hb = np.asarray(hn_beta_vec, dtype=float)
    g = np.array([mp.mpf(float(v)) for v in t["g"]], dtype=object)
    B = np.zeros(off[-1])
    logit = np.full(off[-1], None, dtype=object)
    beta, exists = t["beta"].copy(), t["exists"].copy()
    touched = np.zeros(off[-1], bool)
    lnw = None
    for d in range(D, -1, -1):
        nk = k ** d
        lnw_here, hk = [mp.mpf(0)] * nk, head_key(head, k, d) if len(head) > d and d < D else -1
        for s in range(nk):
            i, c = off[d] + s, cnt[d][s]
            if c.sum() == 0:
                continue
            touched[i] = True
            ex = t["exists"][i] != 0
            b0 = t["beta"][i] if ex else hb
            g0 = mp.mpf(float(t["g"][i])) if ex else mp.mpf(0.0 if d == D else float(hn_g))
            beta[i], exists[i] = b0 + c, 1
            bp, n, lead = np.array(b0, dtype=float), c.copy(), mp.mpf(0)
            if s == hk:
                a = head[d]
                lead = mp.log(mp.mpf(float(b0[a])) / mp.fsum(mp.mpf(float(v)) for v in b0))
                bp[a] += 1.0            # exact: the tests' priors are multiples of 2^-10 far below 2^42
                n[a] -= 1
            L = logdm_exact(bp, n)
            B[i] = row_scale(bp, n) + abs(float(lead))
            if d == D:
                lnw_here[s] = L
                g[i] = mp.mpf(0) if not ex else g[i]
                continue
            ch = [s + c_ * nk for c_ in range(k)]
            S = mp.fsum(lnw[j] for j in ch)
            B[i] += sum(B[off[d + 1] + j] for j in ch)
            if g0 <= 0:
                mix, gn = L, mp.mpf(0)
            elif g0 >= 1:
                mix, gn = S, mp.mpf(1)
            else:
                a_, b_ = mp.log1p(-g0) + L, mp.log(g0) + S
                m = max(a_, b_)
                mix = m + mp.log(mp.exp(a_ - m) + mp.exp(b_ - m))
                gn = mp.exp(b_ - mix)
                logit[i] = b_ - a_
                B[i] += abs(float(mp.log(g0) - mp.log1p(-g0)))
            g[i], lnw_here[s] = gn, lead + mix
        lnw = lnw_here
    return dict(g=g, B=B, beta=beta, exists=exists, touched=touched, logit=logit)


def g_bound(g_exact, B):
    """The first-order image in g of a log-odds error of 64 eps B, plus half an ulp of g and the smallest normal number:
    64 eps B g (1 - g) + 2^-52 g + 2^-1022 (an mpf)."""
    mp = _mp()
    eps = mp.mpf(2) ** -52
    return 64 * eps * mp.mpf(float(B)) * g_exact * (1 - g_exact) + eps * g_exact + mp.mpf(2) ** -1022


def subtree_pow(hn_g, k, D, depth):
    """The reference's price of a full subtree under a missing child of a node at ``depth`` (:757)."""
    m = (k ** (D - depth) - 1) / (k - 1) if k > 1 else float(D - depth)
    return hn_g ** (m - 1)


def map_tables(k, D, t, hn_g):
    """map_leaf (uint8, all levels) of the reference's ``_map_recursion`` (:744-768); the root must exist."""
    off = offsets(k, D)
    ml = np.zeros(off[-1], np.uint8)
    val_child = ex_child = None
    for d in range(D, -1, -1):
        sl = slice(off[d], off[d + 1])
        ex, g = t["exists"][sl] != 0, t["g"][sl]
        if d == D:
            val, leaf = np.ones(k ** d), np.ones(k ** d, bool)
        else:
            stop, thr = 1.0 - g, g * subtree_pow(hn_g, k, D, d)
            prod = np.ones(k ** d)
            for c in range(k):
                cs = slice(c * k ** d, (c + 1) * k ** d)
                prod = prod * np.where(ex_child[cs], val_child[cs], np.where(stop > thr, stop, thr))
            leaf = stop > g * prod
            val = np.where(leaf, stop, g * prod)
        if d > 0:       # missing nodes: the parent's rule, or the full subtree below another missing node
            psl = slice(off[d - 1], off[d])
            pex, pg = np.tile(t["exists"][psl] != 0, k), np.tile(t["g"][psl], k)
            rule = (1.0 - pg > pg * subtree_pow(hn_g, k, D, d - 1)) if d < D else np.ones(k ** d, bool)
            miss = np.where(pex, rule, d == D)
            leaf = np.where(ex, leaf, miss)
        ml[sl] = leaf
        val_child, ex_child = val, ex
    return ml


def path_indices(ctx, k, D):
    """Table indices of the root-to-leaf path of the context ``ctx`` = (x[i-1], x[i-2], ...), at most D symbols."""
    off, key, idx = offsets(k, D), 0, [0]
    for d, c in enumerate(ctx[:D]):
        key += int(c) * k ** d
        idx.append(off[d + 1] + key)
    return idx


# ---- the fixture cases, shared by tests/golden/make_golden_contexttree.py (the reference) and the tests (the drop-in) ----------
def _case(name, k, D, n1, n2, h0_g, seed, h0root=False, hn2=None, same_sample_as=None):
    return dict(name=name, k=k, D=D, n1=n1, n2=n2, h0_g=h0_g, seed=seed, h0root=h0root, hn2=hn2,
                same_sample_as=same_sample_as)


CASES = [
    _case("k2_d3", 2, 3, 300, 100, 0.5, 11),
    _case("k3_d2", 3, 2, 500, 2, 0.3, 12),
    _case("k2_d10", 2, 10, 20000, 5, 0.5, 13),
    _case("k4_d4", 4, 4, 5000, 1, 0.7, 14),
    _case("k2_d4_short", 2, 4, 3, 3, 0.5, 15),
    _case("k3_d3_long", 3, 3, 100000, 0, 0.5, 16),
    _case("n_1", 2, 3, 1, 0, 0.5, 17),
    _case("n_d", 2, 3, 3, 0, 0.5, 18),
    _case("n_d_plus_1", 2, 3, 4, 0, 0.5, 19),
    _case("h0_root", 2, 4, 400, 0, 0.6, 20, h0root=True),
    _case("hn_changed", 3, 3, 600, 300, 0.5, 21, hn2=(0.35, [1.0, 2.0, 1.5])),
    _case("whole", 2, 5, 400, 0, 0.5, 22),
    _case("halves", 2, 5, 200, 200, 0.5, 22, same_sample_as="whole"),
]
TRACE_LEN = 50
STAGES = ("after1", "after2", "final")


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def planted_sample(k, n, rng):
    """An order-2 source with sparse transition rows, so that h_g moves far from the prior."""
    th = rng.dirichlet(np.ones(k) * 0.3, size=(k, k))
    x = np.zeros(n, dtype=np.int64)
    for i in range(2, n):
        x[i] = rng.choice(k, p=th[x[i - 1], x[i - 2]])
    return x


def case_inputs(case):
    """x1, x2, the three contexts of calc_pred_dist and the pred_and_update sequence, all seeded."""
    rng = np.random.default_rng(case["seed"])
    k, D = case["k"], case["D"]
    x = planted_sample(k, case["n1"] + case["n2"], rng)
    ctx = [rng.integers(0, k, D + 3), rng.integers(0, k, D + 1), rng.integers(0, k, 2)]
    return dict(x1=x[:case["n1"]], x2=x[case["n1"]:], ctx0=ctx[0], ctx1=ctx[1], ctx2=ctx[2],
                trace_x=rng.integers(0, k, TRACE_LEN))


def tree_to_tables(root, k, D):
    t = new_tables(k, D)
    off = offsets(k, D)

    def walk(node, s):
        i = off[node.depth] + s
        t["exists"][i], t["g"][i], t["beta"][i], t["leaf"][i] = 1, node.h_g, node.h_beta_vec, node.leaf
        for c, child in enumerate(node.children):
            if child is not None:
                walk(child, s + c * k ** node.depth)
    if root is not None:
        walk(root, 0)
    return t


def map_tree_to_tables(root, k, D):
    """in_tree, leaf (uint8), g and theta (NaN rows where the reference gives None) of an ``estimate_params`` tree."""
    off = offsets(k, D)
    out = dict(in_tree=np.zeros(off[-1], np.uint8), leaf=np.zeros(off[-1], np.uint8), g=np.zeros(off[-1]),
               theta=np.full((off[-1], k), np.nan))

    def walk(node, s):
        i = off[node.depth] + s
        out["in_tree"][i], out["leaf"][i], out["g"][i] = 1, node.leaf, node.h_g
        if node.theta_vec is not None:
            out["theta"][i] = node.theta_vec
        for c, child in enumerate(node.children):
            if child is not None:
                walk(child, s + c * k ** node.depth)
    walk(root, 0)
    return out


def drive(mod, case, inp, make=None):
    """Walk one case through the model package ``mod`` (the reference or the drop-in).  Returns a flat dict of arrays."""
    import copy
    import warnings
    k, D = case["k"], case["D"]
    make = make or mod.LearnModel
    h0_root = mod.GenModel(k, D, h_g=0.8, seed=case["seed"]).gen_params().root if case["h0root"] else None
    m = make(k, D, case["h0_g"], np.arange(1, k + 1) / 2.0, h0_root)
    out = {}

    def snap(stage):
        for name, a in tree_to_tables(m.hn_root, k, D).items():
            out[f"{stage}_{name}"] = a
    # a pred_and_update trace from the prior: the drop-in does the reference's arithmetic step for step
    m0 = copy.deepcopy(m)
    tr = inp["trace_x"]
    out["trace0_p"] = np.stack([m0.pred_and_update(tr[:j + 1], loss="KL").copy() for j in range(len(tr))])
    for name, a in tree_to_tables(m0.hn_root, k, D).items():
        out[f"trace0_{name}"] = a
    m.update_posterior(inp["x1"])
    snap("after1")
    if case["hn2"] is not None:
        m.set_hn_params(case["hn2"][0], np.array(case["hn2"][1]))
    if len(inp["x2"]):
        m.update_posterior(inp["x2"])
        snap("after2")
    for j in range(3):
        mc = copy.deepcopy(m)
        mc.calc_pred_dist(inp[f"ctx{j}"])
        out[f"pred{j}"] = mc.p_theta_vec.copy()
        out[f"pred{j}_argmax"] = np.asarray(mc.make_prediction(loss="0-1"))
        out[f"pred{j}_exists"] = tree_to_tables(mc.hn_root, k, D)["exists"]
    mc = copy.deepcopy(m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, a in map_tree_to_tables(mc.estimate_params(loss="0-1", visualize=False), k, D).items():
            out[f"map_{name}"] = a
    out["trace_p"] = np.stack([m.pred_and_update(tr[:j + 1], loss="KL").copy() for j in range(len(tr))])
    snap("final")
    return out, m


def log_odds_err(g, g_ref, exists):
    """max |g - g_ref| / (g_ref (1 - g_ref)) over the existing nodes with 0 < g_ref < 1; the others must be equal."""
    inner = (exists != 0) & (g_ref > 0) & (g_ref < 1)
    edge = (exists != 0) & ~inner
    assert np.array_equal(g[edge], g_ref[edge])
    if not inner.any():
        return 0.0
    return float(np.max(np.abs(g[inner] - g_ref[inner]) / (g_ref[inner] * (1 - g_ref[inner]))))


def prior_tables(mod, case):
    """The tables of a fresh model of the case (all empty unless the case has an h0_root)."""
    k, D = case["k"], case["D"]
    if not case["h0root"]:
        return new_tables(k, D)
    root = mod.GenModel(k, D, h_g=0.8, seed=case["seed"]).gen_params().root
    # what set_hn_params(h0_root) leaves: the tree itself plus the all-zero context path of its closing calc_pred_dist
    t = tree_to_tables(root, k, D)
    off = offsets(k, D)
    for d in range(D):
        i = off[d]
        if not t["exists"][i]:
            t["exists"][i], t["g"][i], t["beta"][i] = 1, case["h0_g"], np.arange(1, k + 1) / 2.0
    return t


def _stages(mod, case, inp, update):
    """after1 / after2 of the case by ``update(x, t, hn_g, hn_beta_vec)``, which updates the tables ``t`` in place."""
    k, D = case["k"], case["D"]
    off = offsets(k, D)
    t = prior_tables(mod, case)
    g, b = case["h0_g"], np.arange(1, k + 1) / 2.0
    out = {}
    update(inp["x1"], t, g, b)
    out["after1"] = copy_tables(t)
    if case["hn2"] is not None:
        # set_hn_params(hn_g, hn_beta_vec): every existing node, then the all-zero context path of its calc_pred_dist
        g, b = case["hn2"][0], np.array(case["hn2"][1])
        m = t["exists"] != 0
        t["g"][m] = g
        t["g"][off[D]:][m[off[D]:]] = 0.0
        t["beta"][m] = b
        for d in range(D):
            if not t["exists"][off[d]]:
                t["exists"][off[d]], t["g"][off[d]], t["beta"][off[d]] = 1, g, b
    if len(inp["x2"]):
        update(inp["x2"], t, g, b)
        out["after2"] = copy_tables(t)
    return out


def oracle_stages(mod, case, inp):
    """after1 / after2 of the case by ``batch_update`` alone, for the oracle's own check."""
    k, D = case["k"], case["D"]
    return _stages(mod, case, inp, lambda x, t, g, b: batch_update(x, k, D, t, g, b))


def exact_stages(mod, case, inp):
    """``oracle_stages`` by ``batch_update_exact``: after1 / after2 h_g rounded to binary64 (the second update starts from
    the rounded first, as every binary64 implementation does)."""
    k, D = case["k"], case["D"]

    def update(x, t, g, b):
        r = batch_update_exact(level_counts(x, k, D)[D], x[:D], k, D, t, g, b)
        t["g"], t["beta"], t["exists"] = np.array([float(v) for v in r["g"]]), r["beta"], r["exists"]
    return _stages(mod, case, inp, update)


def error_cases(mod, make=None):
    """Boundary cases whose outcome (exception class name and message, or None) is recorded from the reference in
    tests/golden/contexttree_errors.json and replayed against the drop-in."""
    lm = make or mod.LearnModel
    i8 = np.array([0, 1, 1, 0])
    return {
        "ctor_zero_k": lambda: lm(0),
        "ctor_float_k": lambda: lm(2.0),
        "ctor_zero_depth": lambda: lm(2, 0),
        "ctor_float_depth": lambda: lm(2, 1.5),
        "h0_g_above_1": lambda: lm(2, 2, 1.5),
        "h0_g_negative": lambda: lm(2, 2, -0.1),
        "h0_beta_vec_nonpos": lambda: lm(2, 2, 0.5, np.array([1.0, 0.0])),
        "h0_beta_vec_string": lambda: lm(2, 2, 0.5, "a"),
        "h0_root_not_node": lambda: lm(2, 2, 0.5, None, 3),
        "hn_g_above_1": lambda: lm(2).set_hn_params(hn_g=3),
        "hn_beta_vec_negative": lambda: lm(2).set_hn_params(hn_beta_vec=-1.0),
        "hn_root_not_node": lambda: lm(2).set_hn_params(hn_root="tree"),
        "update_float_sample": lambda: lm(2).update_posterior(np.array([0.0, 1.0])),
        "update_list": lambda: lm(2).update_posterior([0, 1]),
        "update_negative": lambda: lm(2).update_posterior(np.array([0, -1, 1])),
        "update_symbol_too_large": lambda: lm(2).update_posterior(np.array([0, 2, 1])),
        "update_negative_and_too_large": lambda: lm(2).update_posterior(np.array([0, 2, -1])),
        "update_ok": lambda: lm(2).update_posterior(i8),
        "estimate_bad_loss": lambda: lm(2).estimate_params(loss="KL", visualize=False),
        "prediction_bad_loss": lambda: lm(2).make_prediction(loss="squared"),
        "pred_dist_2d": lambda: lm(2).calc_pred_dist(np.zeros((2, 2), dtype=int)),
        "pred_dist_float": lambda: lm(2).calc_pred_dist(np.zeros(3)),
        "pred_dist_negative": lambda: lm(2).calc_pred_dist(np.array([0, -1])),
        "pred_dist_too_large": lambda: lm(2).calc_pred_dist(np.array([0, 5])),
        "pred_dist_scalar": lambda: lm(2).calc_pred_dist(1),
        "pred_and_update_2d": lambda: lm(2).pred_and_update(np.zeros((2, 2), dtype=int)),
        "pred_and_update_too_large": lambda: lm(2).pred_and_update(np.array([0, 2])),
        "pred_and_update_bad_loss": lambda: lm(2).pred_and_update(np.array([0, 1]), loss="squared"),
        "gen_ctor_zero_k": lambda: mod.GenModel(0),
        "gen_h_g_above_1": lambda: mod.GenModel(2, h_g=1.2),
        "gen_h_beta_vec_nonpos": lambda: mod.GenModel(2, h_beta_vec=np.array([0.0, 1.0])),
        "gen_h_root_not_node": lambda: mod.GenModel(2, h_root=1),
        "gen_root_not_node": lambda: mod.GenModel(2, root="r"),
        "gen_sample_zero_length": lambda: mod.GenModel(2).gen_sample(0),
        "gen_sample_float_length": lambda: mod.GenModel(2).gen_sample(3.0),
        "gen_initial_values_wrong_len": lambda: mod.GenModel(2, 2).gen_sample(5, initial_values=np.zeros(3, dtype=int)),
        "gen_initial_values_too_large": lambda: mod.GenModel(2, 2).gen_sample(5, initial_values=np.array([0, 2])),
        "gen_initial_values_negative": lambda: mod.GenModel(2, 2).gen_sample(5, initial_values=np.array([0, -2])),
        "gen_sample_ok": lambda: mod.GenModel(2, 2, seed=1).gen_sample(5, initial_values=np.array([0, 1])),
    }


def outcome(fn):
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fn()
    except Exception as e:      # noqa: BLE001 - the outcome IS the exception
        return [type(e).__name__, str(getattr(e, "value", e))]
    return None


def trace_g_ok(g, g_ref, exists, tol, steps=TRACE_LEN):
    """h_g after ``steps`` sequential pred_and_update steps that started ``tol`` apart in log-odds.  A step shifts a node's
    log-odds by log(child mixture / own estimate): the start's error is carried along unchanged, the child mixture brings in
    at most the child's log-odds error (to first order, weights below 1) once per step, and the arithmetic of a step rounds
    g by a few ulp:  |dg| <= g (1 - g) tol (1 + steps) + 8 eps steps."""
    ex = exists != 0
    bound = g_ref[ex] * (1 - g_ref[ex]) * tol * (1 + steps) + 8 * np.finfo(float).eps * steps
    return bool(np.all(np.abs(g[ex] - g_ref[ex]) <= bound))


def trace_p_atol(tol, D, steps=TRACE_LEN):
    """Absolute bound on a predictive probability of a trace that started from a posterior whose h_g are ``tol`` apart in
    log-odds: p is a mixture along one path, |dp| <= sum over the path of |dg|, and by ``trace_g_ok``
    |dg| <= tol (1 + steps) / 4 + 8 eps steps  (g (1 - g) <= 1/4)."""
    return (D + 1) * (tol * (1 + steps) / 4 + 8 * np.finfo(float).eps * steps)
