"""Host restatement of the context-tree batch update on NODE DICTIONARIES (TEST INFRASTRUCTURE ONLY): what
``contexttree_oracle.batch_update`` does on dense tables, for shapes whose dense tables cannot be held (4 ** 13 slots and
up).  A tree is a dict ``{(level, key): [g, beta, leaf]}``; ``key`` packs the context (x[i-1], ..., x[i-level]) with
``bits(k)`` bits per symbol, nearest symbol most significant, in the top ``bits(k) * level`` of ``bits(k) * D`` bits (the
packing of include/ctsp.h, restated here), so that sorting by (level, key) sorts contexts lexicographically.

Canonical node lists, as the fixtures store them: ``level`` (int32), ``ctx`` (uint8 [nodes, D], zero-padded), ``g``,
``beta`` [nodes, k], ``leaf`` (uint8), sorted by (level, ctx).
"""
import numpy as np

from contexttree_oracle import log_odds_err, logdm  # noqa: F401  (re-exported for the tests)

TRACE_LEN = 50


def bits(k):
    return max(1, (k - 1).bit_length())


def pack(ctx, k, D):
    b, key = bits(k), 0
    for j, c in enumerate(ctx):
        key |= int(c) << (b * (D - 1 - j))
    return key


def unpack(key, level, k, D):
    b = bits(k)
    return [(int(key) >> (b * (D - 1 - j))) & ((1 << b) - 1) for j in range(level)]


def level_keys(x, k, D, d):
    """Level-d key of every sample i >= d (int64 array of len(x) - d, or empty)."""
    x = np.asarray(x, dtype=np.int64)
    n, b = len(x), bits(k)
    if n <= d:
        return np.zeros(0, dtype=np.int64)
    key = np.zeros(n - d, dtype=np.int64)
    for j in range(1, d + 1):
        key |= x[d - j:n - j] << (b * (D - j))
    return key


def batch_update(x, k, D, nodes, hn_g, hn_beta_vec):
    """One ``update_posterior(x)`` on the node dict ``nodes``, in place."""
    x = np.asarray(x, dtype=np.int64)
    n, b = len(x), bits(k)
    hb = np.asarray(hn_beta_vec, dtype=float)
    logw = {}
    for d in range(D, -1, -1):
        keys = level_keys(x, k, D, d)
        if len(keys) == 0:
            logw = {}
            continue
        uniq, inv = np.unique(keys, return_inverse=True)
        cnt = np.zeros((len(uniq), k), dtype=np.int64)
        np.add.at(cnt, (inv, x[d:]), 1)
        ex = np.array([(d, int(s)) in nodes for s in uniq])
        b0 = np.array([nodes[(d, int(s))][1] if e else hb for s, e in zip(uniq, ex)], dtype=float).reshape(len(uniq), k)
        g0 = np.array([nodes[(d, int(s))][0] if e else (0.0 if d == D else hn_g) for s, e in zip(uniq, ex)], dtype=float)
        cf = cnt.astype(float)
        if d == D:
            w, newg = logdm(b0, cf), g0
        else:
            shift = b * (D - d - 1)
            S = np.array([sum(logw.get(int(s) | (c << shift), 0.0) for c in range(k)) for s in uniq])
            if d == 0:
                # (bit for bit the dense oracle's sum: NumPy adds the rows of its [k, k^d] table one after another, as
                # above, but sums the single column of the root, [k, 1], in blocks once k >= 8)
                S = np.array([[logw.get(c << shift, 0.0)] for c in range(k)]).sum(0)
            bp, lead = b0.copy(), np.zeros(len(uniq))
            hk = inv[0]                  # sample i = d is the head sample of this level
            lead[hk] = np.log(b0[hk, x[d]] / b0[hk].sum())
            bp[hk, x[d]] += 1
            cf[hk, x[d]] -= 1
            with np.errstate(divide="ignore", invalid="ignore"):
                a_ = np.log1p(-g0) + logdm(bp, cf)
                b_ = np.log(g0) + S
                mix = np.logaddexp(a_, b_)
                newg = np.where(g0 > 0, np.exp(b_ - mix), 0.0)
            w = lead + mix
        logw = {}
        for j, s in enumerate(uniq):
            s = int(s)
            logw[s] = float(w[j])
            leaf = nodes[(d, s)][2] if ex[j] else int(d == D)
            nodes[(d, s)] = [float(newg[j]), b0[j] + cnt[j], leaf]
    return nodes


def map_nodes(k, D, nodes, hn_g):
    """map_leaf of every node of the dict (the root must exist): ``contexttree_oracle.map_tables`` on existing nodes, the
    same products in the same order.  Returns {(level, key): bool}."""
    from contexttree_oracle import subtree_pow
    b, val, ml = bits(k), {}, {}
    for d, s in sorted(nodes, reverse=True):            # children before parents
        if d == D:
            val[(d, s)], ml[(d, s)] = 1.0, True
            continue
        g = nodes[(d, s)][0]
        stop, thr = 1.0 - g, g * subtree_pow(hn_g, k, D, d)
        prod = 1.0
        for c in range(k):
            prod = prod * val.get((d + 1, s | (c << (b * (D - d - 1)))), stop if stop > thr else thr)
        ml[(d, s)] = bool(stop > g * prod)
        val[(d, s)] = stop if ml[(d, s)] else g * prod
    return ml


# ---- canonical lists ---------------------------------------------------------------------------------------------------------
def nodes_to_lists(nodes, k, D):
    order = sorted(nodes)
    m = len(order)
    ctx = np.zeros((m, D), dtype=np.uint8)
    for r, (d, s) in enumerate(order):
        ctx[r, :d] = unpack(s, d, k, D)
    return dict(level=np.array([d for d, _ in order], dtype=np.int32), ctx=ctx,
                g=np.array([nodes[i][0] for i in order], dtype=np.float64),
                beta=np.array([nodes[i][1] for i in order], dtype=np.float64).reshape(m, k),
                leaf=np.array([nodes[i][2] for i in order], dtype=np.uint8))


def lists_to_nodes(t, k, D):
    return {(int(d), pack(c[:d], k, D)): [float(g), np.array(bt, dtype=float), int(lf)]
            for d, c, g, bt, lf in zip(t["level"], t["ctx"], t["g"], t["beta"], t["leaf"])}


def tree_to_nodes(root, k, D):
    """Node dict of a ``_Node`` tree (the reference's or the drop-in's)."""
    nodes = {}
    stack = [(root, ())] if root is not None else []
    while stack:
        node, ctx = stack.pop()
        nodes[(node.depth, pack(ctx, k, D))] = [float(node.h_g), np.array(node.h_beta_vec, dtype=float), int(bool(node.leaf))]
        for c, child in enumerate(node.children):
            if child is not None:
                stack.append((child, ctx + (c,)))
    return nodes


def tree_to_lists(root, k, D):
    return nodes_to_lists(tree_to_nodes(root, k, D), k, D)


def engine_lists(nodes, k, D):
    """Canonical lists of ``SparseCtreePass.get_nodes()`` (level, key, g, beta, leaf): the keys unpacked to contexts."""
    ctx = np.zeros((len(nodes["level"]), D), dtype=np.uint8)
    for r, (d, s) in enumerate(zip(nodes["level"], nodes["key"])):
        ctx[r, :d] = unpack(int(s), int(d), k, D)
    return dict(level=np.asarray(nodes["level"], dtype=np.int32), ctx=ctx, g=np.asarray(nodes["g"]),
                beta=np.asarray(nodes["beta"]), leaf=np.asarray(nodes["leaf"], dtype=np.uint8))


def map_tree_to_lists(root, k, D):
    """level, ctx, leaf, g and theta (NaN rows where the reference gives None) of an ``estimate_params`` tree, sorted."""
    rows = []
    stack = [(root, ())]
    while stack:
        node, ctx = stack.pop()
        th = np.full(k, np.nan) if node.theta_vec is None else np.array(node.theta_vec, dtype=float)
        rows.append((node.depth, pack(ctx, k, D), ctx, int(bool(node.leaf)), float(node.h_g), th))
        for c, child in enumerate(node.children):
            if child is not None:
                stack.append((child, ctx + (c,)))
    rows.sort(key=lambda r: (r[0], r[1]))
    ctx = np.zeros((len(rows), D), dtype=np.uint8)
    for r, row in enumerate(rows):
        ctx[r, :row[0]] = row[2]
    return dict(level=np.array([r[0] for r in rows], dtype=np.int32), ctx=ctx,
                leaf=np.array([r[3] for r in rows], dtype=np.uint8), g=np.array([r[4] for r in rows]),
                theta=np.array([r[5] for r in rows]).reshape(len(rows), k))


def same_node_set(a, b):
    return np.array_equal(a["level"], b["level"]) and np.array_equal(a["ctx"], b["ctx"])


def g_err(a, b):
    """``log_odds_err`` of two canonical lists with the same node set."""
    return log_odds_err(np.asarray(a["g"]), np.asarray(b["g"]), np.ones(len(b["g"]), np.uint8))


# ---- the fixture cases, shared by tests/golden/make_golden_contexttree_sparse.py (the reference) and the tests ----------------
def _case(name, k, D, n1, n2=0, h0_g=0.5, seed=0, h0root=False, map_stored=True):
    return dict(name=name, k=k, D=D, n1=n1, n2=n2, h0_g=h0_g, seed=seed, h0root=h0root, map_stored=map_stored)


CASES = [
    _case("k4_d12", 4, 12, 1500, 700, seed=41),
    _case("k2_d30", 2, 30, 1500, seed=42),
    _case("k3_d20", 3, 20, 1000, h0_g=0.4, seed=43),
    # (the reference's estimate_params did not finish within 30 s on these two: a full subtree per missing node)
    _case("k16_d6", 16, 6, 1500, seed=44, map_stored=False),
    _case("k256_d4", 256, 4, 600, seed=45, map_stored=False),
    _case("k4_d12_n1", 4, 12, 1, seed=46),
    _case("k4_d12_n12", 4, 12, 12, seed=47),
    _case("k4_d12_n13", 4, 12, 13, seed=48),
    _case("k4_d12_h0root", 4, 12, 1500, h0_g=0.6, seed=49, h0root=True),
]


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def planted_sample(k, D, n, rng):
    """Uniform symbols with one motif of 2 D + 5 symbols planted six times, so that nodes at every depth hold more than one
    sample."""
    x = rng.integers(0, k, n).astype(np.int64)
    motif = rng.integers(0, k, 2 * D + 5)
    if n >= 8 * len(motif):
        for start in rng.choice(n - len(motif), 6, replace=False):
            x[start:start + len(motif)] = motif
    return x


def case_inputs(case):
    """x1, x2, the three contexts of calc_pred_dist (the third leaves the tree at once when the tree is deep) and the
    pred_and_update sequence, all seeded."""
    rng = np.random.default_rng(case["seed"])
    k, D = case["k"], case["D"]
    x = planted_sample(k, D, case["n1"] + case["n2"], rng)
    ctx0 = x[:case["n1"]][-(D + 2):]            # the last symbols of x1: a path that exists to the maximal depth
    ctx = [ctx0, rng.integers(0, k, D + 1), rng.integers(0, k, 3)]
    return dict(x1=x[:case["n1"]], x2=x[case["n1"]:], ctx0=ctx[0], ctx1=ctx[1], ctx2=ctx[2],
                trace_x=rng.integers(0, k, TRACE_LEN))


H0_ROOT_SEED = 3        # at h_g = 0.3 most seeds give a root that is a leaf; this one gives a prior tree of 901 nodes


def h0_root_of(mod, case):
    return mod.GenModel(case["k"], case["D"], h_g=0.3, seed=H0_ROOT_SEED).gen_params().root if case["h0root"] else None


def drive(mod, case, inp, make=None):
    """Walk one case through the model package ``mod`` (the reference, or the drop-in with ``make`` =
    ``functools.partial(LearnModel, tables="sparse")``).  Returns a dict of canonical lists and arrays."""
    import copy
    import warnings
    k, D = case["k"], case["D"]
    make = make or mod.LearnModel
    m = make(k, D, case["h0_g"], np.arange(1, k + 1) / 2.0, h0_root_of(mod, case))
    out = {}

    def snap(stage, model):
        for name, a in tree_to_lists(model.hn_root, k, D).items():
            out[f"{stage}_{name}"] = a
    if case["h0root"]:
        snap("prior", m)
    m.update_posterior(inp["x1"])
    snap("after1", m)
    if len(inp["x2"]):
        m.update_posterior(inp["x2"])
        snap("after2", m)
    for j in range(3):
        mc = copy.deepcopy(m)
        mc.calc_pred_dist(inp[f"ctx{j}"])
        out[f"pred{j}"] = mc.p_theta_vec.copy()
        out[f"pred{j}_argmax"] = np.asarray(mc.make_prediction(loss="0-1"))
        out[f"pred{j}_nodes"] = np.asarray(len(tree_to_nodes(mc.hn_root, k, D)))
    if case["map_stored"]:
        mc = copy.deepcopy(m)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name, a in map_tree_to_lists(mc.estimate_params(loss="0-1", visualize=False), k, D).items():
                out[f"map_{name}"] = a
    tr = inp["trace_x"]
    out["trace_p"] = np.stack([m.pred_and_update(tr[:j + 1], loss="KL").copy() for j in range(len(tr))])
    out["final_nodes"] = np.asarray(len(tree_to_nodes(m.hn_root, k, D)))
    return out, m


def planted_tree(mod, k, D):
    """A tree for ``set_hn_params(hn_root=...)`` that takes every branch of the superposition: the all-zero context as a
    chain down to a node at depth D (given h_g = 0.9 there, which the superposition must turn into 0), every other child
    of the chain absent, except that the last child of the root is a leaf above the maximal depth (where a posterior that
    has seen data holds an inner node: a flipped leaf)."""
    node_cls = mod._contexttree._Node
    chain = [node_cls(d, k, 0.15 + 0.05 * d) for d in range(D + 1)]
    for d, node in enumerate(chain):
        node.h_beta_vec[:] = np.arange(1, k + 1) + d / 4.0
        if d < D:
            node.children[0] = chain[d + 1]
    chain[D].h_g = 0.9
    if k > 1 and D > 1:
        flipped = node_cls(1, k, 0.35)
        flipped.h_beta_vec[:] = 3.0
        flipped.leaf = True
        chain[0].children[k - 1] = flipped
    return chain[0]


def extended_drive(mod, case, inp, make=None):
    """``drive``, then on its model: superpose ``planted_tree``, pickle and unpickle, one more ``pred_and_update`` and the
    MAP tree.  Returns ``drive``'s dict with these stages added."""
    import pickle
    import warnings
    k, D = case["k"], case["D"]
    out, m = drive(mod, case, inp, make=make)

    def snap(stage, model):
        for name, a in tree_to_lists(model.hn_root, k, D).items():
            out[f"{stage}_{name}"] = a
    m.set_hn_params(hn_root=planted_tree(mod, k, D))
    snap("planted", m)
    out["planted_p"] = m.p_theta_vec.copy()
    m = pickle.loads(pickle.dumps(m))
    snap("unpickled", m)
    out["unpickled_p"] = m.pred_and_update(inp["trace_x"][:D + 1], loss="KL").copy()
    snap("unpickled_after", m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, a in map_tree_to_lists(m.estimate_params(loss="0-1", visualize=False), k, D).items():
            out[f"planted_map_{name}"] = a
    return out, m


# ---- c_k = 1 with an absent child: tests/golden/make_golden_contexttree_k1.py (the reference) and the tests ------------------
K1_CASES = [dict(name="k1_d2", D=2, h0_g=0.7, n=0), dict(name="k1_d3", D=3, h0_g=0.7, n=0),
            dict(name="k1_d2_stops_above", D=2, h0_g=0.3, n=0), dict(name="k1_d2_one_symbol", D=2, h0_g=0.9, n=1)]


def k1_drive(mod, case, make=None):
    """A fresh c_k = 1 model.  With n = 0 it is given a root that is not a leaf and whose only child is absent: the
    superposition creates the child (and the closing calc_pred_dist the all-zero path above the maximal depth), so the node
    at depth D - 1 exists and its child at depth D is missing.  With n = 1 it learns one symbol instead: the root alone
    exists.  Returns JSON-ready lists: the posterior, and the MAP tree or the outcome of ``estimate_params``."""
    from contexttree_oracle import outcome
    D = case["D"]
    m = (make or mod.LearnModel)(1, D, case["h0_g"], np.array([1.5]))
    if case["n"]:
        m.update_posterior(np.zeros(case["n"], dtype=int))
    else:
        root = mod._contexttree._Node(0, 1, 0.9)
        root.h_beta_vec[:] = 2.5
        m.set_hn_params(hn_root=root)
    posterior, got = {n: a.tolist() for n, a in tree_to_lists(m.hn_root, 1, D).items()}, {}
    what = outcome(lambda: got.update(map_tree_to_lists(m.estimate_params(loss="0-1", visualize=False), 1, D)))
    return dict(posterior=posterior, map_outcome=what, map={n: a.tolist() for n, a in got.items()})


def stage_lists(fx, stage):
    return {name: fx[f"{stage}_{name}"] for name in ("level", "ctx", "g", "beta", "leaf")}


def oracle_stages(case, inp, prior=None):
    """after1 / after2 of the case by ``batch_update``, from the canonical lists ``prior`` (None: an empty tree)."""
    k, D = case["k"], case["D"]
    nodes = lists_to_nodes(prior, k, D) if prior is not None else {}
    g, b = case["h0_g"], np.arange(1, k + 1) / 2.0
    out = {}
    batch_update(inp["x1"], k, D, nodes, g, b)
    out["after1"] = nodes_to_lists(nodes, k, D)
    if len(inp["x2"]):
        batch_update(inp["x2"], k, D, nodes, g, b)
        out["after2"] = nodes_to_lists(nodes, k, D)
    return out
