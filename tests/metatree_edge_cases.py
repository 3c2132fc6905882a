"""Forests, states and samples for the edge tests of the meta-tree engine (TEST INFRASTRUCTURE; needs no GPU).

Everything is built from seeds.  A case is a dict: ``tabs`` (the structure tables of ``_mtree.FlatForest``), ``fam``,
``degree``, ``h0``, ``dim_cont`` / ``dim_cat`` / ``cat_card``, ``state`` (the tables before the update), ``xc`` / ``xk`` /
``y``, and ``claims``: what the case is about, in numbers that ``tests/test_metatree.py`` re-derives without a GPU (the exact
g strictly inside (0, 1), |t| beyond exp's range, which slabs are empty, the side of the LDS predicate), so that a GPU test
cannot pass on a case that does not reach the branch it names.

Trees are over continuous features in [0, 1): a node splits feature ``depth % dims`` of its box in the middle.
"""
import numpy as np

import metatree_oracle as orc

H0 = {orc.BERNOULLI: [0.5, 0.5], orc.POISSON: [1.0, 1.0, 0.0], orc.EXPONENTIAL: [1.0, 1.0],
      orc.NORMAL: [0.0, 1.0, 1.0, 1.0, 0.0]}
LDS_SLOTS, MAX_SLABS, MIN_SPAN, WAVE = 6144, 64, 1024, 64          # include/mtree.h, _mtree.py (pinned in test_metatree.py)


def h0_of(fam, degree=0):
    return np.full(degree, 0.5) if fam == orc.CATEGORICAL else np.array(H0[fam])


# ---- forests ------------------------------------------------------------------------------------------------------------------
def _pack(tree_off, feat, child0, nchild, thr_off, depth, thr):
    i32 = lambda a: np.array(a, np.int32)       # noqa: E731
    return dict(tree_off=i32(tree_off), feat=i32(feat), child0=i32(child0), nchild=i32(nchild), thr_off=i32(thr_off),
                depth=i32(depth), thr=np.array(thr, dtype=np.float64))


def heap_tree(n_nodes, dims=1, n_trees=1):
    """Binary trees in heap order (children of v: 2v + 1, 2v + 2 where they exist), breadth-first by construction;
    2^(d+1) - 1 nodes make the full tree of depth d."""
    feat, child0, nchild, thr_off, dep, thr, tree_off = [], [], [], [], [], [], [0]
    for _ in range(n_trees):
        base = len(feat)
        box = [np.tile([0.0, 1.0], (dims, 1))]
        for v in range(n_nodes):
            d = int(np.log2(v + 1))
            dep.append(d)
            kids = [c for c in (2 * v + 1, 2 * v + 2) if c < n_nodes]
            if not kids:
                feat.append(-1), child0.append(0), nchild.append(0), thr_off.append(-1)
                continue
            k = d % dims
            lo, hi = box[v][k]
            mid = (lo + hi) / 2
            feat.append(k), child0.append(base + kids[0]), nchild.append(len(kids)), thr_off.append(len(thr))
            thr.extend([lo, mid, hi] if len(kids) == 2 else [lo, hi])
            for side in range(len(kids)):
                b = box[v].copy()
                if len(kids) == 2:
                    b[k] = (lo, mid) if side == 0 else (mid, hi)
                box.append(b)
        tree_off.append(len(feat))
    return _pack(tree_off, feat, child0, nchild, thr_off, dep, thr)


def binary_tree(depth, dims=1, n_trees=1):
    return heap_tree(2 ** (depth + 1) - 1, dims, n_trees)


def grow_one_child(tabs):
    """The last node of a one-tree forest (a leaf, the last of the deepest level) gets one child over its whole range:
    one node more, breadth-first order kept."""
    assert len(tabs["tree_off"]) == 2 and tabs["feat"][-1] < 0
    t = {k: v.copy() for k, v in tabs.items()}
    last = len(t["feat"]) - 1
    t["feat"][last], t["child0"][last], t["nchild"][last], t["thr_off"][last] = 0, last + 1, 1, len(t["thr"])
    t["thr"] = np.concatenate([t["thr"], [0.0, 1.0]])
    for k, v in (("feat", -1), ("child0", 0), ("nchild", 0), ("thr_off", -1), ("depth", t["depth"][last] + 1)):
        t[k] = np.append(t[k], np.int32(v))
    t["tree_off"] = np.array([0, last + 2], np.int32)
    return t


def chain(depth):
    """2 depth + 1 nodes: at every level a leaf on the left and, on the right, the node that goes on.  The node of depth d
    splits [1 - 2^-d, 1) in the middle, so x >= 1 - 2^-depth reaches the deepest leaf."""
    feat, child0, nchild, thr_off, dep, thr = [], [], [], [], [], []
    for v in range(2 * depth + 1):
        d = (v + 1) // 2
        dep.append(d)
        if (v == 0 or v % 2 == 0) and d < depth:
            lo = 1.0 - 2.0 ** -d
            feat.append(0), child0.append(2 * d + 1), nchild.append(2), thr_off.append(len(thr))
            thr.extend([lo, (lo + 1.0) / 2, 1.0])
        else:
            feat.append(-1), child0.append(0), nchild.append(0), thr_off.append(-1)
    return _pack([0, 2 * depth + 1], feat, child0, nchild, thr_off, dep, thr)


def star(nchild, categorical=False):
    """A root with ``nchild`` leaves: continuous thresholds 0, 1, ..., nchild (exact in float32), or categorical."""
    feat = [0] + [-1] * nchild
    return _pack([0, nchild + 1], feat, [1] + [0] * nchild, [nchild] + [0] * nchild, [-1 if categorical else 0] + [-1] * nchild,
                 [0] + [1] * nchild, [] if categorical else np.arange(nchild + 1.0))


def stumps(n_trees):
    """``n_trees`` trees of three nodes; tree b splits [0, 1) at (b + 1) / (n_trees + 1)."""
    feat, child0, nchild, thr_off, dep, thr, tree_off = [], [], [], [], [], [], [0]
    for b in range(n_trees):
        feat.extend([0, -1, -1]), child0.extend([3 * b + 1, 0, 0]), nchild.extend([2, 0, 0])
        thr_off.extend([3 * b, -1, -1]), dep.extend([0, 1, 1]), thr.extend([0.0, (b + 1) / (n_trees + 1), 1.0])
        tree_off.append(3 * b + 3)
    return _pack(tree_off, feat, child0, nchild, thr_off, dep, thr)


def start_state(tabs, fam, degree=0, g0=0.5):
    nodes, B = len(tabs["feat"]), len(tabs["tree_off"]) - 1
    return dict(g=np.where(tabs["feat"] < 0, 0.0, g0), post=np.tile(h0_of(fam, degree), (nodes, 1)), lml=np.full(nodes, np.nan),
                lcm=np.zeros(nodes), prob=np.ones(B) / B)


def _case(name, tabs, fam, xc, xk, y, degree=0, state=None, cat_card=(), **claims):
    xc = None if xc is None else np.asarray(xc, dtype=np.float64).reshape(len(y), -1)
    xk = None if xk is None else np.asarray(xk).reshape(len(y), -1)
    return dict(name=name, tabs=tabs, fam=fam, degree=degree, h0=h0_of(fam, degree), dim_cont=0 if xc is None else xc.shape[1],
                dim_cat=0 if xk is None else xk.shape[1], cat_card=list(cat_card), xc=xc, xk=xk, y=np.asarray(y),
                state=start_state(tabs, fam, degree) if state is None else state, claims=claims)


def in_leaf(j, n_leaves, rng, size):
    """x in the inside of leaf j of a one-feature full binary tree with n_leaves leaves."""
    return (j + rng.uniform(0.05, 0.95, size)) / n_leaves


# ---- conditioning of the real columns -----------------------------------------------------------------------------------------
CONDITIONING = ("level", "outlier_1", "outlier_1e6", "outlier_1e12", "scales", "constant")


def conditioning(kind, fam, n=200, seed=0):
    """One depth-3 binary tree (leaf j = [j, j + 1) / 8), real-valued y (normal or exponential):

    level        y = 1e6 + j + 0.01 |z| in leaf j: a large common level
    outlier_V    row 0 alone in leaf 0 with y = V, every other row 1e-3 (1 + 0.1 z) in leaves 1..7
    scales       leaf j holds 10^(3j - 9) (1 + 0.1 z): twenty-one orders of magnitude between the leaves; row 0 lies in leaf 7
    constant     leaf 3 holds one value, 0.1 (level 1) or 1e6 + 0.1, in every row; the other leaves 1 + j + 0.1 z
    """
    rng = np.random.default_rng([seed, CONDITIONING.index(kind), n])
    leaf = rng.integers(0, 8, n)
    z = np.abs(rng.standard_normal(n)) if fam == orc.EXPONENTIAL else rng.standard_normal(n)
    if kind == "level":
        y = 1e6 + leaf + 0.01 * z
    elif kind.startswith("outlier"):
        leaf = rng.integers(1, 8, n)
        leaf[0] = 0
        y = 1e-3 * (1 + 0.1 * z)
        y[0] = float(kind.split("_")[1])
    elif kind == "scales":
        leaf[:8] = np.arange(8)[::-1]
        y = 10.0 ** (3 * leaf - 9) * (1 + 0.1 * z)
    else:
        leaf[:3] = 3
        y = np.where(leaf == 3, 0.1 if seed % 2 == 0 else 1e6 + 0.1, 1.0 + leaf + 0.1 * np.abs(z))
    x = in_leaf(leaf, 8, rng, n)
    return _case(f"{kind}-{orc_name(fam)}-n{n}-s{seed}", binary_tree(3), fam, x, None, y, leaf=leaf)


def orc_name(fam):
    return {v: k for k, v in orc.FAMILY.items()}[fam]


def nan_rows(fam, n=200, seed=0):
    """A depth-3 tree over two features (feature depth % 2): rows with x0 = NaN stop at the root, rows with x1 = NaN at a
    depth-1 node, so inner nodes have rows of their own beside their children's."""
    rng = np.random.default_rng([seed, 77])
    x = rng.random((n, 2))
    x[::9, 0] = np.nan
    x[4::11, 1] = np.nan
    leaf = np.floor(np.nan_to_num(x[:, 0]) * 4).astype(int)
    # (the leaves differ little and the rows lie where the prior expects them: every h_g stays inside (0, 1))
    y = {orc.NORMAL: 0.3 * leaf + rng.standard_normal(n), orc.EXPONENTIAL: rng.exponential(1.0 + 0.1 * leaf),
         orc.POISSON: rng.poisson(1.0 + 0.2 * leaf)}[fam]
    own_root = int(np.isnan(x[:, 0]).sum())
    own_d1 = int((~np.isnan(x[:, 0]) & np.isnan(x[:, 1])).sum())
    return _case(f"nan-{orc_name(fam)}", binary_tree(3, dims=2), fam, x, None, y, own_root=own_root, own_d1=own_d1)


# ---- the mixture ----------------------------------------------------------------------------------------------------------------
# (1 - 2^-53 and nextafter(1, 0) are the same binary64 number)
G0 = (0.0, 1.0, 5e-324, 1e-300, 2.0 ** -53, 0.5, float(np.nextafter(1.0, 0.0)))


def mixture(fam, g0, sign, n=4000, seed=0):
    """Four depth-2 trees of 7 nodes.  In tree 0 the depth-1 nodes 1 and 2 have h_g = g0; node 1 gets ``n`` rows whose two
    leaves disagree (left y = 0, right y = 1; normal: -5 and 5), node 2 gets 100 rows.  sign = -1: fresh leaves, so the
    children explain the rows far better than node 1 does and t = ln(1 - g) + lml - ln g - sum L is far below -745 for
    every g0 inside (0, 1).  sign = +1: the leaves' posteriors have seen 1000 rows of the opposite kind before, the
    children are far worse and t is far above 745.  Tree 1 has h_g = 0 at every node and a root that has seen rows of
    another kind (its root's own lml only: it ends more than 745 below tree 0), tree 2 is tree 0 with prior probability
    0, tree 3 is tree 0 with 0.25 at the root, so that prob[0] / prob[3] holds the root's L to the oracle."""
    rng = np.random.default_rng([seed, fam, int(sign > 0)])
    tabs = binary_tree(2, n_trees=4)
    st = start_state(tabs, fam)
    for base in (0, 14, 21):
        st["g"][base + 1] = st["g"][base + 2] = g0
    st["g"][7:14] = 0.0
    st["g"][21] = 0.25
    st["prob"] = np.array([0.5, 0.25, 0.0, 0.25])
    x = np.concatenate([rng.uniform(0.0, 0.5, n), rng.uniform(0.5, 1.0, 100)])
    right = (np.floor(x * 4).astype(int) % 2) == 1
    if fam == orc.BERNOULLI:
        y = right.astype(np.int64)
        seen = {False: [1000.5, 0.5], True: [0.5, 1000.5]}          # [ones, zeros]: the leaf has seen the other leaf's rows
    else:
        y = np.where(right, 5.0, -5.0) + 0.1 * rng.standard_normal(len(x))
        seen = {False: [50.0, 1001.0, 501.0, 6.0, 1000.0], True: [-50.0, 1001.0, 501.0, 6.0, 1000.0]}
    st["post"][7] = [2000.5, 0.5] if fam == orc.BERNOULLI else seen[False]
    if sign > 0:
        for base in (0, 14, 21):
            st["post"][base + 3], st["post"][base + 4] = seen[False], seen[True]
    return _case(f"mixture-{orc_name(fam)}-g{g0!r}-{'+' if sign > 0 else '-'}", tabs, fam, x, None, y, state=st, g0=g0, sign=sign,
                 node=1)


# ---- limits and table edges ---------------------------------------------------------------------------------------------------
def wide_continuous(seed=0):
    """A 16-way continuous root: rows on every threshold 0..16 (a row on threshold i belongs to child i; 16 to the last),
    -inf, +inf, -0.0, NaN, and rows inside every child.  All values are exact in float32."""
    rng = np.random.default_rng([seed, 16])
    x = np.concatenate([np.arange(17.0), [-np.inf, np.inf, -0.0, np.nan, -3.0, 40.0], rng.integers(0, 64, 200) / 4.0])
    y = (rng.random(len(x)) < 0.3 + 0.02 * np.nan_to_num(x, posinf=16, neginf=0).clip(0, 16)).astype(np.int64)
    return _case("wide-continuous", star(16), orc.BERNOULLI, x, None, y)


def wide_categorical(card=16, seed=0):
    """A 16-way categorical root; with card > 16 the feature has values that no child takes: such a row stops at the root
    and is no bad value."""
    rng = np.random.default_rng([seed, card])
    xk = np.concatenate([np.arange(card), rng.integers(0, card, 300)])
    y = rng.poisson(1.0 + xk % 5)
    return _case(f"wide-categorical-{card}", star(16, categorical=True), orc.POISSON, None, xk, y, cat_card=[card],
                 outside=int((xk >= 16).sum()))


def lds_edge(fam, n_nodes, degree=0, n=600, seed=0):
    """A one-tree forest with exactly ``n_nodes`` nodes: the heap tree of the largest odd count, then one-child steps."""
    rng = np.random.default_rng([seed, n_nodes])
    odd = n_nodes if n_nodes % 2 else n_nodes - 1
    if n_nodes in (2048, 2049):
        odd = 2047
    tabs = heap_tree(odd)
    for _ in range(n_nodes - odd):
        tabs = grow_one_child(tabs)
    x = rng.random(n)
    grid = (np.arange(8192) + 0.5) / 8192
    hit = grid[orc.stops(orc.route(tabs, 1, grid[:, None], None))[0] == n_nodes - 1]
    x[:40] = rng.choice(hit, 40)                        # rows for the last node (the grown one, where there is one)
    if fam == orc.CATEGORICAL:
        y = (np.floor(x * 64).astype(int) + rng.integers(0, 3, n)) % degree
    else:
        y = rng.poisson(1 + 5 * x)
    ni, nr, _ = stat_cols(fam, degree)
    cols = ni + min(nr, 1)
    return _case(f"lds-{orc_name(fam)}-{n_nodes}", tabs, fam, x, None, y, degree=degree, cols=cols,
                 lds=bool(n_nodes * cols <= LDS_SLOTS))


def stat_cols(fam, degree=0):
    from bayesml_amd import _mtree
    return _mtree.stat_cols(fam, degree)


def deep_chain(fam, depth=24, n=300, seed=0):
    rng = np.random.default_rng([seed, depth, fam])
    x = 1.0 - 2.0 ** -rng.integers(0, depth + 3, n).astype(np.float64) * rng.uniform(0.5, 1.0, n)
    x[:5] = 1.0 - 2.0 ** -(depth + 2)
    x[5] = np.nan
    y = ((rng.random(n) < 0.5 + 0.4 * (x > 0.9)).astype(np.int64) if fam == orc.BERNOULLI
         else 2.0 + np.nan_to_num(x) + 0.1 * rng.standard_normal(n))
    return _case(f"chain-{depth}-{orc_name(fam)}", chain(depth), fam, x, None, y, deepest=int((x >= 1 - 2.0 ** -depth).sum()))


def many_trees(n_trees=1024, n=257, seed=0):
    rng = np.random.default_rng([seed, n_trees])
    x = rng.random(n)
    return _case(f"stumps-{n_trees}", stumps(n_trees), orc.BERNOULLI, x, None, (rng.random(n) < x).astype(np.int64))


# ---- the global-scratch table: one wave rewrites the same entries round after round -------------------------------------------
def rewrite(fam, n=4096, seed=0):
    """A depth-11 tree over two features (4095 nodes: global scratch for 2 columns and more).  Row i goes to one of four
    leaves, leaf (i + i // 64) % 4 of the four, so every 64-row round of a wave adds to the same four entries and a
    different lane leads each group from round to round; every 17th row stops at the root (x0 = NaN), every 19th at a
    depth-1 node (x1 = NaN)."""
    rng = np.random.default_rng([seed, fam, 11])
    i = np.arange(n)
    which = (i + i // 64) % 4
    cx = np.array([0.1, 0.3, 0.6, 0.9])[which] + rng.uniform(0, 1e-4, n)      # a leaf is 1/64 wide in either feature
    cy = np.array([0.2, 0.7, 0.4, 0.8])[which] + rng.uniform(0, 1e-4, n)
    x = np.stack([cx, cy], axis=1)
    x[::17, 0] = np.nan
    x[::19, 1] = np.nan
    y = rng.poisson(2.0 + which) if fam == orc.POISSON else 1e3 * (which + 1) + rng.standard_normal(n)
    return _case(f"rewrite-{orc_name(fam)}", binary_tree(11, dims=2), fam, x, None, y, which=which)


# ---- slabs --------------------------------------------------------------------------------------------------------------------
def slab_spans(n, S):
    """[lo, hi) of every slab, by the kernel's arithmetic (slab_of in csrc/mtree_kernels.h)."""
    span = -(-n // S)
    span = -(-span // WAVE) * WAVE
    return [(s * span, max(s * span, min(s * span + span, n))) for s in range(S)]


def slabs(fam, n, seed=0):
    rng = np.random.default_rng([seed, fam, n])
    x = rng.random(n)
    y = (rng.random(n) < x).astype(np.int64) if fam == orc.BERNOULLI else 1e3 + np.floor(x * 4) + 0.1 * rng.standard_normal(n)
    return _case(f"slabs-{orc_name(fam)}-{n}", binary_tree(2), fam, x, None, y)


# ---- predict on hand-set states -----------------------------------------------------------------------------------------------
def predict_case(fam, n, degree=0, seed=0, symmetric=False):
    """Three trees (depth 3 over two features, depth 2, a stump) with random positive posteriors, h_g random in (0, 1) with
    one inner node at 0 and one at 1 in every tree, one tree with probability 0; rows with a NaN feature stop at inner
    nodes.  exponential: some nodes have alpha <= 1; normal: some alpha <= 1 (nu <= 2): their mean / variance is NaN."""
    rng = np.random.default_rng([seed, fam, n, degree])
    parts = [binary_tree(3, dims=2), binary_tree(2, dims=2), binary_tree(1, dims=2), binary_tree(2, dims=2)]
    tabs, off, toff = {k: [] for k in orc.STRUCT}, 0, 0
    tree_off = [0]
    for p in parts:
        m = len(p["feat"])
        tabs["feat"].append(p["feat"]), tabs["nchild"].append(p["nchild"]), tabs["depth"].append(p["depth"])
        tabs["child0"].append(np.where(p["feat"] >= 0, p["child0"] + off, 0))
        tabs["thr_off"].append(np.where(p["feat"] >= 0, p["thr_off"] + toff, -1))
        tabs["thr"].append(p["thr"])
        off, toff = off + m, toff + len(p["thr"])
        tree_off.append(off)
    tabs = _pack(tree_off, *(np.concatenate(tabs[k]) for k in ("feat", "child0", "nchild", "thr_off", "depth", "thr")))
    nodes = off
    inner = np.flatnonzero(tabs["feat"] >= 0)
    g = np.where(tabs["feat"] >= 0, rng.uniform(0.05, 0.95, nodes), 0.0)
    for b in range(len(parts)):
        mine = inner[(inner >= tree_off[b]) & (inner < tree_off[b + 1])]
        g[mine[0]] = [1.0, 0.3, 0.0, 0.6][b]               # roots: pass everything down, mix, stop at the root, mix
        if len(mine) > 2:
            g[mine[1]], g[mine[2]] = 0.0, 1.0
    if fam == orc.BERNOULLI:
        post = rng.uniform(0.5, 20.0, (nodes, 2))
        if symmetric:
            post[:, 1] = post[:, 0]
    elif fam == orc.CATEGORICAL:
        post = rng.uniform(0.5, 20.0, (nodes, degree))
    elif fam == orc.POISSON:
        post = np.stack([rng.uniform(0.5, 50, nodes), rng.uniform(0.5, 20, nodes), rng.uniform(0, 30, nodes)], axis=1)
    elif fam == orc.EXPONENTIAL:
        post = np.stack([rng.uniform(1.5, 30, nodes), rng.uniform(0.5, 20, nodes)], axis=1)
        post[[7, 8, 18, 31], 0] = [1.0, 0.5, 0.999, 1.0]                     # leaves of trees 0, 1 and 3
    else:
        post = np.stack([rng.uniform(1, 2, nodes), rng.uniform(0.5, 20, nodes), rng.uniform(1.5, 20, nodes),
                         rng.uniform(0.5, 5, nodes), rng.integers(0, 30, nodes).astype(float)], axis=1)
        post[[7, 8, 18, 31], 2] = [1.0, 0.5, 0.75, 1.0]
    prob = np.array([0.5, 0.3, 0.0, 0.2])
    x = rng.random((n, 2))
    x[3::7, 0] = np.nan
    x[5::11, 1] = np.nan
    st = dict(g=g, post=post, lml=np.full(nodes, np.nan), lcm=np.zeros(nodes), prob=prob)
    return _case(f"predict-{orc_name(fam)}-n{n}", tabs, fam, x, None, np.zeros(n), degree=degree, state=st)
