"""Forests and samples of the linear-regression edge cases (TEST INFRASTRUCTURE ONLY): the smallest shapes at which the
ordering, the segmented Gram pass and the sweep of include/mtree.h can go wrong.  tests/test_metatree_lr.py checks without a
GPU that each case reaches what it names; tests/test_gpu_metatree_lr.py runs them on the device.

A tree is given as a nested spec: ``None`` is a leaf, ``(feature, thresholds, children)`` an inner node (``thresholds``: the
inner cut points of a continuous feature, ``None`` for a categorical one).  Continuous ranges are (-10, 10).
"""
import numpy as np

import metatree_lr_oracle as lro

LO, HI = -10.0, 10.0


def forest(specs):
    """The flat tables (``_mtree.FlatForest``'s fields) of a list of tree specs, nodes breadth-first."""
    out = {k: [] for k in ("feat", "child0", "nchild", "thr_off", "depth", "thr")}
    tree_off = [0]
    for spec in specs:
        order, base = [(spec, 0)], len(out["feat"])
        for node, depth in order:
            out["depth"].append(depth)
            if node is None:
                for k, v in (("feat", -1), ("child0", 0), ("nchild", 0), ("thr_off", -1)):
                    out[k].append(v)
                continue
            feat, cuts, kids = node
            out["feat"].append(feat)
            out["child0"].append(base + len(order))
            out["nchild"].append(len(kids))
            if cuts is None:
                out["thr_off"].append(-1)
            else:
                assert len(cuts) == len(kids) - 1
                out["thr_off"].append(len(out["thr"]))
                out["thr"].extend([LO, *cuts, HI])
            order.extend((c, depth + 1) for c in kids)
        tree_off.append(len(out["feat"]))
    return dict(tree_off=np.array(tree_off, np.int32), thr=np.array(out["thr"], np.float64),
                **{k: np.array(out[k], np.int32) for k in ("feat", "child0", "nchild", "thr_off", "depth")})


ROOT_ONLY = None
STUMP = (0, [0.0], [None, None])                        # x0 < 0 | x0 >= 0


def full_binary(depth, lo=-4.0, hi=4.0):
    """A full binary tree that halves (lo, hi) of x0 at every level."""
    if depth == 0:
        return None
    mid = 0.5 * (lo + hi)
    return (0, [mid], [full_binary(depth - 1, lo, mid), full_binary(depth - 1, mid, hi)])


def sample(n, D, seed, x0=None, noise=1.0, offset=0.0, intercept=True, dtype=np.float64):
    """n rows of D regressors: centred features (plus ``offset``), the last a column of ones when ``intercept`` and D > 1;
    ``x0`` (an array) fixes the first column, which the forests above route on.  y = x . theta + noise."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, size=(n, D)) + offset
    if x0 is not None:
        x[:, 0] = x0
    if intercept and D > 1:
        x[:, -1] = 1.0
    x = x.astype(dtype)
    theta = np.linspace(1.0, -1.0, D) if D > 1 else np.array([1.5])
    y = x.astype(np.float64) @ theta + noise * rng.standard_normal(n)
    return x, y


def case(name, specs, x, y, D=None, xk=None, dim_cat=0, cat_card=(), h0=None, g=None, prob=None):
    tabs = forest(specs)
    D = x.shape[1] if D is None else D
    h0 = lro.default_h0(D) if h0 is None else h0
    g0 = np.where(tabs["feat"] < 0, 0.0, 0.5) if g is None else g
    return dict(name=name, tabs=tabs, D=D, dim_cont=D, dim_cat=dim_cat, cat_card=np.array(cat_card, dtype=np.int32), h0=h0,
                state=lro.initial_state(tabs, D, h0, g0, prob), xc=x, xk=xk, y=y)


def quad_padding(n):
    """D = 1, a root-only tree: fewer rows than a quad, exactly one, one more."""
    x, y = sample(n, 1, seed=n)
    return case(f"quad_n{n}", [ROOT_ONLY], x, y)


def tile_edge(D, dtype):
    """The tile's last columns: D = 14 leaves one zero column, D = 15 none; x as float32 is widened on the device."""
    x, y = sample(200, D, seed=D, dtype=dtype)
    return case(f"tile_D{D}_{np.dtype(dtype).name}", [STUMP], x, y)


def block_edge(kind, block):
    """Runs against the block boundary of the sorted array (the left leaf's rows come first)."""
    left, right = {"crossing": (block + 5, 37), "ending": (block, 37), "three_blocks": (2 * block + 3, 10)}[kind]
    rng = np.random.default_rng(left)
    x0 = np.concatenate([rng.uniform(-2, -0.1, left), rng.uniform(0.1, 2, right)])
    x, y = sample(left + right, 3, seed=left + 1, x0=x0)
    return case(f"block_{kind}", [STUMP], x, y), (left, right)


def scattered(block):
    """The rows of each leaf scattered through the batch, over several slabs and blocks."""
    n = 3 * block + 17
    x, y = sample(n, 3, seed=7)
    return case("scattered", [STUMP], x, y)


def tiny_runs():
    """A depth-4 binary tree, 64 rows, all with x0 < 0.5: many runs of a few rows, the right-most leaves empty."""
    rng = np.random.default_rng(11)
    x, y = sample(64, 2, seed=12, x0=rng.uniform(-4, 0.5, 64))
    return case("tiny_runs", [full_binary(4)], x, y)


def mixed_routing():
    """A three-way continuous root with a categorical and a binary node below it, and a categorical root."""
    rng = np.random.default_rng(13)
    x, y = sample(300, 2, seed=14, intercept=False)
    xk = rng.integers(0, 3, size=(300, 1))
    x[::7, 0] = -1.0                                   # rows exactly on a threshold go right
    specs = [(0, [-1.0, 1.0], [None, (2, None, [None, None, None]), (1, [0.5], [None, None])]),
             (2, None, [None, None, (0, [-0.5, 0.25], [None, None, None])])]
    g = np.where(forest(specs)["feat"] < 0, 0.0, 0.5)
    g[0], g[9] = 0.7, 0.3
    return case("mixed_routing", specs, x, y, xk=xk.astype(np.int64), dim_cat=1, cat_card=[3], g=g, prob=[0.4, 0.6])


def several_trees():
    """Three trees of different shape: prob_vec."""
    x, y = sample(400, 3, seed=15)
    return case("several_trees", [ROOT_ONLY, STUMP, full_binary(2, -2.0, 2.0)], x, y)


def precision_edge():
    """Features offset by 5 with an intercept, noise sd 0.01: cond_2(Lambda) of 1e4..1e5, and beta cancels."""
    x, y = sample(500, 3, seed=16, noise=0.01, offset=5.0)
    x[:, :2] = 5.0 + (x[:, :2] - 5.0) / 6.0
    x[:250, 0], x[250:, 0] = -np.abs(x[:250, 0]), np.abs(x[250:, 0])
    y = x @ np.linspace(1.0, -1.0, 3) + 0.01 * np.random.default_rng(17).standard_normal(500)
    return case("precision_edge", [STUMP], x, y)


def second_stage(first, n=50, seed=18):
    """A second sample for the forest of ``first``."""
    x, y = sample(n, first["D"], seed=seed)
    out = dict(first)
    out.update(name=first["name"] + "_stage2", xc=x, y=y,
               xk=None if first["xk"] is None else np.random.default_rng(seed).integers(0, 3, size=(n, 1)))
    return out
