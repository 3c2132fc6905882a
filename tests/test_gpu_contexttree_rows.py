"""The context-tree sweep on the MI355X against an exact (mpmath) evaluation of the same update.

``ctree_sweep`` reads the deepest level's counts from device memory, so a test writes any count table and any
``beta`` / ``g`` / ``exists`` state and sweeps: every branch of ``dm_row_and_update`` (rising factorial, lgamma, Stirling's
series, the per-symbol difference form on a prior that is already large, the head sample through each of them) and every
branch of the mixture is hit on purpose.  lnW is not exposed; the observable is h_g above the deepest level,
logit g' = logit g0 + sum_children lnW - lnDM(own row).

The bound (``orc.g_bound``).  B(s) is the sum over the subtree of s of the sizes of the terms that are added:
row_scale + |logit g0| + |lead| per touched node.  A child's error passes through the two-way mixture with weights that
sum to 1, so the subtree sum is the scale of a node's log-odds error; the project's "64 eps of the case" gives
delta = 64 eps B(s), whose first-order image in g is delta g (1 - g) (a comparison of logits means nothing next to 1):

    |g' - g*| <= 64 eps B(s) g* (1 - g*) + 2^-52 g* + 2^-1022.

h_beta_vec, the node set, the entries of nodes without samples and a second sweep from the same state are bit for bit.
Every case prints ``err / bound``; the figures of an MI355X, with the parent commit's on the large-prior rows, are in
profiles/ctree_rows.md.
"""
import itertools

import numpy as np
import pytest
import torch

import contexttree_oracle as orc

pytestmark = pytest.mark.gpu

SENT_G, SENT_B = 0.123, 7.25          # what the entries of nodes that do not exist hold before a sweep
_ENGINES = {}


def _pass(k, D):
    from bayesml_amd import _ctree
    if (k, D) not in _ENGINES:
        _ENGINES[k, D] = _ctree.CtreePass(k, D, torch.device("cuda", 0))
    return _ENGINES[k, D]


# ---- cases ---------------------------------------------------------------------------------------------------------------
def new_case(k, D, hn_g=0.5, hn_beta=None, head=()):
    n = orc.offsets(k, D)[-1]
    return dict(k=k, D=D, hn_g=hn_g, hn_beta=np.full(k, 0.5) if hn_beta is None else np.asarray(hn_beta, dtype=float),
                head=[int(v) for v in head], cnt=np.zeros((k ** D, k), np.int64),
                t=dict(g=np.full(n, SENT_G), beta=np.full((n, k), SENT_B), exists=np.zeros(n, np.uint8),
                       leaf=np.zeros(n, np.uint8)))


def put(case, d, s, beta, g):
    """Node s of level d exists with this state."""
    i = orc.offsets(case["k"], case["D"])[d] + s
    case["t"]["exists"][i], case["t"]["g"][i], case["t"]["beta"][i] = 1, g, np.asarray(beta, dtype=float)


def other_prior(k, base):
    return base + 0.5 * (np.arange(k) % 3)


def sweep(case):
    k, D = case["k"], case["D"]
    eng = _pass(k, D)
    eng.set_tables(case["t"])
    eng._out[2:] = torch.from_numpy(case["cnt"].reshape(-1)).cuda()
    eng.sweep(torch.tensor(case["head"], dtype=torch.int32, device="cuda"), case["hn_g"], case["hn_beta"])
    return eng.get_tables()


def check(case, label, saturated=False):
    """Sweeps the case twice and holds it to ``batch_update_exact``.  Returns the largest err / bound.  Unless the case is
    ``saturated`` on purpose, some node must end with h_g in (1e-290, 1 - 1e-12): a case whose h_g are all 0 or 1 would
    pass whatever lnDM the kernel computed.  (Next to 0 binary64 keeps the relative precision of h_g, so the bound still
    checks the log-odds there; next to 1 it does not.)"""
    mp = orc._mp()
    k, D, t = case["k"], case["D"], case["t"]
    want = orc.batch_update_exact(case["cnt"], case["head"], k, D, t, case["hn_g"], case["hn_beta"])
    got, again = sweep(case), sweep(case)
    for name in ("g", "beta", "exists"):
        assert np.array_equal(got[name], again[name]), (label, name, "two sweeps differ")
    assert np.array_equal(got["exists"], want["exists"]), label
    assert np.array_equal(got["beta"], want["beta"]), label
    quiet = ~want["touched"]
    assert np.array_equal(got["g"][quiet], t["g"][quiet]), (label, "a node without samples was written")
    oD, worst, lines = orc.offsets(k, D)[D], 0.0, []
    for i in np.flatnonzero(want["touched"]):
        if i >= oD:
            assert got["g"][i] == float(want["g"][i]), (label, i)          # 0 at creation, untouched afterwards
            continue
        err = abs(mp.mpf(float(got["g"][i])) - want["g"][i])
        ratio = float(err / orc.g_bound(want["g"][i], want["B"][i]))
        lines.append(f"node {i}: g* = {float(want['g'][i]):.17g}, B = {want['B'][i]:.3e}, err / bound = {ratio:.3g}")
        worst = max(worst, ratio)
    print(f"{label}: err / bound = {worst:.3g}")
    inner = [i for i in np.flatnonzero(want["touched"]) if i < oD and 1e-290 < want["g"][i] < 1 - 1e-12]
    assert saturated or inner, (label, "every h_g of the case is saturated", lines)
    for line in lines:
        print("    " + line)
    assert worst <= 1.0, (label, lines)
    return worst


# ---- the catalogue of rows: (name, prior, counts) ---------------------------------------------------------------------------
def _sparse256():
    return [0] * 250 + [1, 2, 63, 64, 65, 10000]


H2, BIG = [0.5, 0.5], 1e6 + 0.5
ROWS = [
    ("small", H2, [3, 2]),
    ("tot64_direct", H2, [40, 24]),
    ("tot65", H2, [40, 25]),
    ("v63.5_64.5", H2, [63, 64]),
    ("post_total_64", H2, [31, 32]),
    ("post_total_63", H2, [31, 31]),
    ("one_symbol", H2, [1000, 0]),
    ("skewed_log1p", H2, [100000, 7]),
    ("n1e7", H2, [6000000, 4000000]),
    ("k3_mixed", [1.0, 2.0, 1.5], [500, 3, 70]),
    ("k256_even", [0.5] * 256, [40000] * 256),
    ("k256_sparse", [0.5] * 256, _sparse256()),
    ("tiny_beta", [1e-3, 1e-3], [500, 0]),
    ("big_n100", [BIG, BIG], [60, 40]),
    ("big_n1e4", [BIG, BIG], [6000, 4000]),
    ("big_n64_direct", [BIG, BIG], [64, 0]),
    ("big_skewed_n65", [BIG, 3.5], [64, 1]),
    ("big1e7_k4_n1e3", [1e7 + 0.5] * 4, [250, 251, 249, 250]),
    ("b100_n1e6", [100.5, 80.5], [600000, 400000]),
    ("b64_n65", [64.0, 64.0], [65, 0]),
]
ROW_IDS = [r[0] for r in ROWS]


def neighbour_prior(n, k, j):
    """A prior of strength 2^j shaped like the counts (never the row's own): multiples of 2^-10."""
    n = np.asarray(n, dtype=float)
    shape = (n / n.sum() + 1.0 / k) * (1.0 + (np.arange(k) % 3) / 8.0)
    return np.maximum(np.round(2.0 ** j * shape * 1024.0), 1.0) / 1024.0


def centred(build, b):
    """``build(prior)`` with the neighbours' prior chosen, and then the root's g0 (hn_g where the root does not exist),
    such that the root's exact new h_g is near 1/2, or small but far from underflow.  A row is checked through
    logit g' = logit g0 + S - L: were that far above 0, or below -745, g' would be 1 or 0 whatever lnDM the kernel
    computed.  The neighbours' prior runs through strengths 2^-4, 2^-2, ... until |S - L| <= 600; g0 then takes up a
    positive S - L (down to e^-600) and most of a negative one (a g0 within 1e-13 of 1 would itself have no digits)."""
    mp = orc._mp()
    for j in range(-4, 40, 2):
        prior = neighbour_prior(build.n, len(b), j)
        case = build(prior)
        assert not np.array_equal(prior, np.asarray(b, dtype=float))
        lo = orc.batch_update_exact(case["cnt"], case["head"], case["k"], case["D"], case["t"], case["hn_g"],
                                    case["hn_beta"])["logit"][0]         # built with g0 = 1/2: this is S - L
        if -600 <= lo <= 600:
            g0 = float(1 / (1 + mp.exp(lo))) if lo > -30 else 0.5          # (h_g = e^lo >= 1e-261 keeps its digits)
            if case["t"]["exists"][0]:
                case["t"]["g"][0] = g0
            else:
                case["hn_g"] = g0
            return case
    raise AssertionError("no neighbour prior brings S - L into range")


def deep_case(b, n, missing):
    """The row at child 0 of a D = 1 tree (child 1 exists without samples, the others do not exist); the root's prior is
    another one (``centred``), so that S - L is neither an exact 0 nor out of h_g's range."""
    k = len(b)

    def build(prior):
        c = new_case(k, 1, hn_g=0.4, hn_beta=b if missing else other_prior(k, 1.25))
        c["cnt"][0] = n
        if not missing:
            put(c, 1, 0, b, 0.0)
        put(c, 1, 1, other_prior(k, 3.25), 0.0)
        put(c, 0, 0, prior, 0.5)
        return c
    build.n = n
    return centred(build, b)


def own_case(b, n, missing, head=()):
    """The row as the own row of the root of a D = 1 tree: the counts are split over children 0 and 1, whose prior is
    another one (``centred``).  With a head symbol a the root evaluates (b + e_a, n)."""
    k = len(b)
    n = np.asarray(n, dtype=np.int64)

    def build(prior):
        c = new_case(k, 1, hn_g=0.5, hn_beta=b if missing else other_prior(k, 1.25), head=head)
        c["cnt"][0], c["cnt"][1] = n // 3, n - n // 3
        put(c, 1, 0, prior, 0.0)
        put(c, 1, 1, prior, 0.0)
        if not missing:
            put(c, 0, 0, b, 0.5)
        return c
    build.n = n
    return centred(build, b)


@pytest.mark.parametrize("missing", [False, True], ids=["existing", "missing"])
@pytest.mark.parametrize("name,b,n", ROWS, ids=ROW_IDS)
def test_row_at_the_deepest_level(name, b, n, missing):
    check(deep_case(b, n, missing), f"deep {name} {'missing' if missing else 'existing'}")


@pytest.mark.parametrize("missing", [False, True], ids=["existing", "missing"])
@pytest.mark.parametrize("name,b,n", ROWS, ids=ROW_IDS)
def test_row_as_an_upper_nodes_own_row(name, b, n, missing):
    check(own_case(b, n, missing), f"own {name} {'missing' if missing else 'existing'}")


# ---- the head sample ---------------------------------------------------------------------------------------------------------
HEAD_ROWS = [
    ("direct", H2, [10, 5]),
    ("direct_edge", H2, [40, 24]),          # 64 samples besides the head: still the rising factorial
    ("series_edge", H2, [40, 25]),
    ("series", H2, [101, 50]),
    ("big_diff", [BIG, BIG], [6000, 4000]),
    ("big_skewed", [BIG, 3.5], [64, 1]),
    ("big_direct", [BIG, BIG], [60, 4]),
    ("k4_big", [1e7 + 0.5] * 4, [250, 251, 249, 250]),
]


@pytest.mark.parametrize("missing", [False, True], ids=["existing", "missing"])
@pytest.mark.parametrize("where", ["hot", "cold"])
@pytest.mark.parametrize("name,b,n", HEAD_ROWS, ids=[r[0] for r in HEAD_ROWS])
def test_head_sample_on_the_root(name, b, n, where, missing):
    """n_head = D = 1: the root's counts are the child sums plus the head symbol, and it evaluates (b + e_a, n)."""
    a = int(np.argmax(n)) if where == "hot" else int(np.argmin(n))
    check(own_case(b, n, missing, head=[a]), f"head {name} {where} {'missing' if missing else 'existing'}")


D2_TABLES = {
    "series": [[40, 25], [3, 2], [100000, 7], [63, 64]],        # level 1: (100040, 32) and (66, 66)
    "direct": [[3, 2], [10, 5], [0, 0], [20, 9]],               # level 1: (3, 2) and (30, 14); key 2 has no samples
}


@pytest.mark.parametrize("head", [(), (0,), (1,), (0, 1), (1, 0), (1, 1), (0, 0)], ids=lambda h: "head" + "".join(map(str, h)))
@pytest.mark.parametrize("table", list(D2_TABLES))
def test_head_samples_at_two_levels(table, head):
    """k = 2, D = 2, n_head in {0, 1, 2}: head[0] ends at the root, head[1] at the level-1 node of key head[0], whose
    lead + mix goes into the root.  Node 1 of level 1 does not exist yet; the others do, every level with its own prior."""
    c = new_case(2, 2, hn_g=0.35, hn_beta=[1.0, 0.25], head=head)
    c["cnt"][:] = D2_TABLES[table]
    for s in range(4):
        put(c, 2, s, [0.5 + 0.25 * s, 0.75], 0.0)
    put(c, 1, 0, [2.5, 1.5], 0.3)
    put(c, 0, 0, [1.5, 0.5], 0.7)
    check(c, f"D2 {table} head={head}")


def test_head_on_a_large_prior_at_level_one():
    """The head sample through the difference form one level above the leaves (k = 3, D = 2)."""
    for head in ((2, 0), (1, 1), (0,)):
        c = new_case(3, 2, hn_g=0.5, hn_beta=[0.5, 1.0, 1.5], head=head)
        rng = np.random.default_rng(5)
        c["cnt"][:] = rng.integers(0, 400, (9, 3))
        for s in range(9):
            put(c, 2, s, [1e5 + 0.5 + s, 2e5 + 0.25, 3.5], 0.0)
        for s in range(3):
            put(c, 1, s, [3e5 + 0.5, 5e5 + 1.5 * s, 80.5], 0.2 + 0.3 * s)
        put(c, 0, 0, [1e6 + 0.5, 2e6 + 0.5, 250.5], 0.5)
        check(c, f"D2 k3 large prior head={head}")


# ---- the mixture -----------------------------------------------------------------------------------------------------------------
G0 = [0.0, 1e-300, 1e-9, 0.5, 1 - 1e-9, 1.0]
HN_G = [0.0, 0.5, 1.0]


@pytest.mark.parametrize("root_missing", [False, True], ids=["root_exists", "root_missing"])
@pytest.mark.parametrize("hn_g", HN_G)
@pytest.mark.parametrize("i", range(len(G0)))
def test_mixture_values(i, hn_g, root_missing):
    """k = 3, D = 2.  Level 1: node 0 exists with g0 = G0[i], node 1 does not exist (g0 = hn_g), node 2 exists without
    samples.  The root exists with g0 = G0[i + 3] or does not exist."""
    c = new_case(3, 2, hn_g=hn_g, hn_beta=[0.5, 1.0, 1.5], head=(1, 2))
    rng = np.random.default_rng(100 + i)
    c["cnt"][:] = rng.integers(0, 6, (9, 3))          # few samples: S - L stays within a few nats of 0
    c["cnt"][3] = [7, 0, 2]
    c["cnt"][[2, 5, 8]] = 0
    for s in (0, 3, 4, 2):
        put(c, 2, s, [1.0, 2.0, 1.5], 0.0)
    put(c, 1, 0, [2.0, 0.5, 0.5], G0[i])
    put(c, 1, 2, [4.0, 4.5, 5.0], 0.77)
    if not root_missing:
        put(c, 0, 0, [0.75, 0.75, 2.0], G0[(i + 3) % len(G0)])
    # g0 = 0 and g0 = 1 are fixed points and 1e-300 stays below 1e-290: a case made of these alone is saturated by design
    used = [G0[i], hn_g, hn_g if root_missing else G0[(i + 3) % len(G0)]]
    check(c, f"mixture g0={G0[i]!r} hn_g={hn_g} {'root missing' if root_missing else 'root exists'}",
          saturated=all(v in (0.0, 1e-300, 1.0) for v in used))


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("i", range(len(G0)))
def test_mixture_values_other_alphabets(k, i):
    c = new_case(k, 2, hn_g=0.5, hn_beta=other_prior(k, 0.5), head=(k - 1, 0))
    rng = np.random.default_rng(200 + 10 * k + i)
    c["cnt"][:] = rng.integers(0, 6, (k * k, k))
    c["cnt"][k - 1::k] = 0                            # level 1's last node gets the head sample and nothing else
    for s in range(0, k * k, 2):
        put(c, 2, s, other_prior(k, 1.0), 0.0)
    for s in range(k):
        put(c, 1, s, other_prior(k, 2.0 + s), G0[(i + s) % len(G0)])
    put(c, 0, 0, other_prior(k, 0.25), G0[(i + 2) % len(G0)])
    used = [G0[(i + s) % len(G0)] for s in range(k)] + [G0[(i + 2) % len(G0)]]
    check(c, f"mixture k={k} g0 from {G0[i]!r}", saturated=all(v in (0.0, 1e-300, 1.0) for v in used))


def test_mixture_tie():
    """A - B == 0 exactly: g0 = 1/2, one child with the root's prior and all the counts, no head sample."""
    c = new_case(2, 1)
    c["cnt"][0] = [70, 30]
    put(c, 1, 0, [1.5, 2.5], 0.0)
    put(c, 0, 0, [1.5, 2.5], 0.5)
    check(c, "mixture tie")


def test_mixture_saturates_both_ways():
    """|A - B| > 745.  Children that explain the sample far better than the root: g' rounds to 1; children whose priors
    are badly wrong: g' underflows to 0."""
    c = new_case(2, 1)
    c["cnt"][0], c["cnt"][1] = [1000, 0], [0, 1000]
    put(c, 0, 0, [0.5, 0.5], 0.5)
    check(c, "mixture towards 1", saturated=True)
    assert sweep(c)["g"][0] == 1.0
    c = new_case(2, 1)
    c["cnt"][0], c["cnt"][1] = [1000, 0], [1000, 0]
    put(c, 1, 0, [0.5, 1000.5], 0.0)
    put(c, 1, 1, [0.5, 1000.5], 0.0)
    put(c, 0, 0, [0.5, 0.5], 0.5)
    check(c, "mixture towards 0", saturated=True)
    assert sweep(c)["g"][0] == 0.0


# ---- values at the scale the engine is timed at, through the public class --------------------------------------------------
def _walk(k, n, p, seed):
    """An order-1 source: the symbol advances by one with probability p."""
    return np.cumsum(np.random.default_rng(seed).random(n) < p) % k


def _update_and_check(m, x, label):
    """One update_posterior held to the exact update of the tables the device had before it; the entries of nodes
    without samples keep their bits."""
    mp = orc._mp()
    k, D = m.c_k, m.c_d_max
    eng = m._eng()
    before = eng.get_tables()
    if not m._has_root:
        before["exists"][:] = 0          # (the first update clears the node set)
    want = orc.batch_update_exact(orc.level_counts(x, k, D)[D], x[:D], k, D, before, m.hn_g, m.hn_beta_vec)
    m.update_posterior(x)
    got = eng.get_tables()
    ex, quiet = want["exists"] != 0, ~want["touched"]
    assert np.array_equal(got["exists"], want["exists"]), label
    assert np.array_equal(got["beta"][ex], want["beta"][ex]), label
    for name in ("g", "beta", "exists"):
        assert np.array_equal(got[name][quiet], before[name][quiet]), (label, name, "a node without samples was written")
    worst = 0.0
    for i in np.flatnonzero(want["touched"]):
        err = abs(mp.mpf(float(got["g"][i])) - want["g"][i])
        worst = max(worst, float(err / orc.g_bound(want["g"][i], want["B"][i])))
    print(f"{label}: {int(want['touched'].sum())} nodes, err / bound = {worst:.3g}")
    assert worst <= 1.0, label
    return want


def _same_bits(m, xs, label):
    """A second model given the same updates ends with the same bits in every table."""
    from bayesml_amd import contexttree
    m2 = contexttree.LearnModel(m.c_k, m.c_d_max, device="cuda:0")
    for x in xs:
        m2.update_posterior(x)
    a, b = m._eng().get_tables(), m2._eng().get_tables()
    ex = a["exists"] != 0
    assert np.array_equal(a["exists"], b["exists"]) and np.array_equal(a["leaf"], b["leaf"]), label
    assert np.array_equal(a["g"][ex], b["g"][ex]) and np.array_equal(a["beta"][ex], b["beta"][ex]), label


def _check_pred_dist(m, want, rng, label):
    """calc_pred_dist on three contexts: (a) to 64 eps relative against the exact mixture along the path of the tables the
    device holds; (b) against the mixture of the exact h_g: p is linear in each g with a coefficient of at most 1 (a
    difference of two probabilities), so |dp| <= sum over the path of the nodes' bounds, plus (a)'s 64 eps p."""
    mp = orc._mp()
    k, D = m.c_k, m.c_d_max
    eps = mp.mpf(2) ** -52
    t = m._eng().get_tables()
    for length in (D + 3, D + 1, 2):
        x = rng.integers(0, k, length)
        idx = orc.path_indices(x[:-1][::-1], k, D)
        # (a node of the path that does not exist yet takes the defaults, as in the reference)
        there = [bool(t["exists"][i]) for i in idx]
        default_g = [mp.mpf(0.0 if d == D else float(m.hn_g)) for d in range(len(idx))]

        def mixture(g):
            g = [v if e else dg for v, e, dg in zip(g, there, default_g)]
            beta = [[mp.mpf(float(v)) for v in (t["beta"][i] if e else m.hn_beta_vec)] for i, e in zip(idx, there)]
            p = [v / mp.fsum(beta[-1]) for v in beta[-1]]
            for d in range(len(idx) - 2, -1, -1):
                p = [(1 - g[d]) * v / mp.fsum(beta[d]) + g[d] * q for v, q in zip(beta[d], p)]
            return p
        got = m.calc_pred_dist(x).p_theta_vec.copy()
        own = mixture([mp.mpf(float(t["g"][i])) for i in idx])
        exact = mixture([want["g"][i] for i in idx])
        slack = mp.fsum(orc.g_bound(want["g"][i], want["B"][i]) for i in idx)
        ra = max(float(abs(mp.mpf(float(a)) - b) / (64 * eps * b)) for a, b in zip(got, own))
        rb = max(float(abs(mp.mpf(float(a)) - b) / (64 * eps * b + slack)) for a, b in zip(got, exact))
        print(f"{label} context of {length - 1}: err / (64 eps p) = {ra:.3g}; against the exact h_g err / bound = {rb:.3g}")
        assert ra <= 1.0 and rb <= 1.0, (label, length)


def test_workload_scale_k2_d6_with_second_updates():
    """N = 2e6 at (2, 6), then 500 and 5000 symbols more on the trained model: a batch far smaller than the counts it lands
    on, at every node of the tree."""
    from bayesml_amd import contexttree
    x = _walk(2, 2_000_000 + 5500, 0.3, 61)
    parts = [x[:2_000_000], x[2_000_000:2_000_500], x[2_000_500:]]
    m = contexttree.LearnModel(2, 6, device="cuda:0")
    want = _update_and_check(m, parts[0], "(2, 6) N = 2e6")
    assert want["touched"].all()
    _same_bits(m, parts[:1], "(2, 6) N = 2e6")             # (before calc_pred_dist, which writes the rows of its path)
    _check_pred_dist(m, want, np.random.default_rng(62), "(2, 6) N = 2e6")
    _update_and_check(m, parts[1], "(2, 6) + 500")
    want = _update_and_check(m, parts[2], "(2, 6) + 5000")
    _check_pred_dist(m, want, np.random.default_rng(63), "(2, 6) + 5000")


def _steps(k, n, seed):
    """An order-1 source that reaches every context: the symbol advances by 0..k-1 with falling probabilities."""
    p = 0.5 ** np.arange(1, k + 1)
    return np.cumsum(np.random.default_rng(seed).choice(k, n, p=p / p.sum())) % k


@pytest.mark.parametrize("source", ["walk", "steps"])
def test_workload_scale_k4_d3(source):
    """N = 2e6 at (4, 3).  The walk advances by 0 or 1, so it reaches 29 of the 85 nodes (the others must keep their
    bits); the second source advances by any step and reaches them all."""
    from bayesml_amd import contexttree
    x = _walk(4, 2_000_000, 0.4, 64) if source == "walk" else _steps(4, 2_000_000, 66)
    m = contexttree.LearnModel(4, 3, device="cuda:0")
    want = _update_and_check(m, x, f"(4, 3) N = 2e6 {source}")
    assert int(want["touched"].sum()) == (29 if source == "walk" else 85)
    _same_bits(m, [x], f"(4, 3) N = 2e6 {source}")
    _check_pred_dist(m, want, np.random.default_rng(65), f"(4, 3) N = 2e6 {source}")


# ---- the MAP sweep on all small trees ------------------------------------------------------------------------------------------
def _all_patterns(k, D):
    """Every upward-closed node set that contains the root, as uint8 tables."""
    off = orc.offsets(k, D)

    def subtrees(d, s):          # the sets of table indices a subtree rooted at (d, s) can occupy, the node included
        if d == D:
            return [[off[d] + s]]
        per_child = [[[]] + subtrees(d + 1, s + c * k ** d) for c in range(k)]
        return [[off[d] + s] + sum(combo, []) for combo in itertools.product(*per_child)]
    out = []
    for nodes in subtrees(0, 0):
        e = np.zeros(off[-1], np.uint8)
        e[nodes] = 1
        out.append(e)
    return out


def _random_patterns(k, D, count, rng):
    off = orc.offsets(k, D)
    out = []
    for _ in range(count):
        e = np.zeros(off[-1], np.uint8)
        e[0] = 1
        for d in range(1, D + 1):
            parent = np.tile(e[off[d - 1]:off[d]], k)           # child c of key s is key s + c k^(d-1)
            e[off[d]:off[d + 1]] = parent & (rng.random(k ** d) < 0.6)
        out.append(e)
    return out


@pytest.mark.parametrize("k,D", [(2, 3), (3, 2), (2, 1), (1, 3)])
def test_map_sweep_on_small_trees(k, D):
    """map_leaf bit for bit against the oracle's ``map_tables``: every node set of the two smallest shapes, 300 seeded
    random ones of the others; h_g from {0, 0.3, 0.5, 0.7, 1} and random values with hn_g in {0, 0.5, 1}, whose powers are
    exact (the ties 1 - g == g prod and stop == thr are reproducible), and random h_g with a generic hn_g."""
    eng, rng = _pass(k, D), np.random.default_rng(1000 * k + D)
    patterns = _all_patterns(k, D) if (k, D) in ((2, 1), (1, 3)) else _random_patterns(k, D, 300, rng)
    assert len(patterns) == (4 if (k, D) in ((2, 1), (1, 3)) else 300)
    n, seen = eng.nodes, set()
    for e in patterns:
        for hn_g in (0.0, 0.5, 1.0, 0.37):
            g = rng.random(n)
            if hn_g != 0.37:
                pick = rng.random(n) < 0.75
                g[pick] = rng.choice([0.0, 0.3, 0.5, 0.7, 1.0], int(pick.sum()))
            t = dict(g=g, beta=np.ones((n, k)), exists=e, leaf=np.zeros(n, np.uint8))
            eng.set_tables(t)
            got, want = eng.map_leaf(hn_g), orc.map_tables(k, D, t, hn_g)
            assert np.array_equal(got, want), (k, D, hn_g, e.tolist(), g.tolist())
            seen.add(want.tobytes())
    assert len(seen) >= (2 if D == 1 else 4)          # the cases do not all end in the same tree
