"""The index arithmetic of ``contexttree.LearnModel`` on sparse storage (``tables="sparse"``, ``_ctsp.SparseCtreePass``):
nodes are addressed by ``(level, key)`` instead of a dense table index.  Each function is the sparse twin of the method of
``LearnModel`` it is named after and is called from there with the model as first argument.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _ctsp
from .._engine import EngineLimitError
from .._exceptions import ResultWarning

# estimate_params refuses to build a MAP tree of more nodes than this (a missing node under hn_g = 1 is the root of a full
# subtree of (k^(D-d+1) - 1) / (k - 1) nodes); the count is taken before a single node is built.
MAX_MAP_NODES = 1 << 20


def make_engine(model):
    make = model._ctree_pass_factory
    return make(model.c_k, model.c_d_max) if make is not None else _ctsp.SparseCtreePass(model.c_k, model.c_d_max,
                                                                                         model._device)


def _node_dict(nodes):
    """{(level, key): [g, beta, leaf]} of ``get_nodes`` arrays."""
    return {(int(d), int(s)): [float(g), np.array(b, dtype=float), int(lf)]
            for d, s, g, b, lf in zip(nodes["level"], nodes["key"], nodes["g"], nodes["beta"], nodes["leaf"])}


def _node_arrays(nd, k):
    """``get_nodes`` arrays of a node dict, in canonical order."""
    order = sorted(nd)
    return dict(level=np.array([d for d, _ in order], dtype=np.int32), key=np.array([s for _, s in order], dtype=np.int64),
                g=np.array([nd[i][0] for i in order], dtype=np.float64),
                beta=np.array([nd[i][1] for i in order], dtype=np.float64).reshape(len(order), k),
                leaf=np.array([nd[i][2] for i in order], dtype=np.uint8))


def hn_root(model, node_cls):
    """The posterior as the reference's ``_Node`` tree, children in symbol order."""
    k, D = model.c_k, model.c_d_max
    nodes = model._eng().get_nodes()
    b = _ctsp.symbol_bits(k)
    made = {}
    root = None
    for d, s, g, beta, lf in zip(nodes["level"], nodes["key"], nodes["g"], nodes["beta"], nodes["leaf"]):
        d, s = int(d), int(s)
        node = node_cls(d, k, float(g))
        node.h_beta_vec[:] = beta
        node.leaf = bool(lf)
        made[(d, s)] = node
        if d == 0:
            root = node
        else:
            made[(d - 1, _ctsp.parent_key(s, d, k, D))].children[(s >> (b * (D - d))) & ((1 << b) - 1)] = node
    return root


def scatter_tree(model, nd, d, s, orig):
    """ref:547-576 on the node dict ``nd``: superpose ``orig`` on the existing node (d, s)."""
    k, D = model.c_k, model.c_d_max
    if orig is None:
        low = (1 << (_ctsp.symbol_bits(k) * (D - d))) - 1
        for (dd, ss), row in nd.items():
            if dd >= d and (ss & ~low) == s:
                row[0] = model._default_g(dd)
                row[1] = np.array(model.hn_beta_vec, dtype=float)
        return
    # (an explicit stack: a tree may be 63 levels deep, and the None branch above must not run once per descendant)
    stack = [(d, s, orig)]
    while stack:
        d, s, orig = stack.pop()
        if orig is None:
            scatter_tree(model, nd, d, s, None)
            continue
        row = nd[(d, s)]
        row[0], row[1] = float(orig.h_g), np.array(orig.h_beta_vec, dtype=float)
        if d == D:
            row[2], row[0] = 1, 0.0
        elif orig.leaf:
            row[2] = 1
        else:
            row[2] = 0
            for c in range(k):
                cs = _ctsp.child_key(s, d, c, k, D)
                if (d + 1, cs) not in nd:
                    nd[(d + 1, cs)] = [0.5, np.full(k, 0.5), 0]
                stack.append((d + 1, cs, orig.children[c]))


def set_hn_root(model, hn_root_):
    eng = model._eng()
    if not model._has_root:
        eng.clear()
        nd = {(0, 0): [0.5, np.full(model.c_k, 0.5), 0]}
    else:
        nd = _node_dict(eng.get_nodes())
    scatter_tree(model, nd, 0, 0, hn_root_)
    eng.set_nodes(_node_arrays(nd, model.c_k))
    model._has_root = True


def path(model, x):
    """The D + 1 (or fewer) nodes that the context before x[-1] selects, missing ones with the defaults as ref:956-965.
    Returns ([(level, key)], g, beta, leaf)."""
    k, D = model.c_k, model.c_d_max
    i = x.shape[0] - 1
    depth = min(i, D)
    ctx = [int(x[i - d - 1]) for d in range(depth)]
    idx = [(d, _ctsp.key_of(ctx[:d], k, D)) for d in range(depth + 1)]
    g, beta, exists, leaf = model._eng().gather(idx)
    g, beta, leaf = g.copy(), beta.copy(), leaf.copy()
    for d in range(depth + 1):
        if not exists[d]:
            g[d], beta[d], leaf[d] = model._default_g(d), model.hn_beta_vec, d == D
    return idx, g, beta, leaf


def _full_subtree_nodes(k, height):
    """Nodes of a full k-ary tree of ``height`` levels below its root."""
    return height + 1 if k == 1 else (k ** (height + 1) - 1) // (k - 1)


def _subtree_pow(hn_g, k, D, depth):
    m = (k ** (D - depth) - 1) / (k - 1) if k > 1 else float(D - depth)
    return hn_g ** (m - 1) if hn_g > 0 or m > 1 else 1.0


def map_tree(model, node_cls):
    """The MAP tree (ref:733-831) from ``ctsp_map``'s flags; only the pruned tree is built, and its size is counted first."""
    k, D, hn_g = model.c_k, model.c_d_max, model.hn_g
    eng = model._eng()
    ml = eng.map_leaf(hn_g)
    nodes = eng.get_nodes()
    nd = {(int(d), int(s)): (float(g), b, bool(m)) for d, s, g, b, m in zip(nodes["level"], nodes["key"], nodes["g"],
                                                                            nodes["beta"], ml)}

    def missing_is_leaf(d, parent_g):
        """A missing child at depth d of an existing node: the parent's rule (ref:755-762)."""
        return d == D or 1.0 - parent_g > parent_g * _subtree_pow(hn_g, k, D, d - 1)

    # the size first: existing internal nodes are walked, a missing child is one leaf or one full subtree
    total, stack = 0, [(0, 0)]
    while stack:
        d, s = stack.pop()
        g, _, is_leaf = nd[(d, s)]
        total += 1
        if is_leaf:
            continue
        for c in range(k):
            cs = _ctsp.child_key(s, d, c, k, D)
            if (d + 1, cs) in nd:
                stack.append((d + 1, cs))
            else:
                total += 1 if missing_is_leaf(d + 1, g) else _full_subtree_nodes(k, D - d - 1)
        if total > MAX_MAP_NODES:
            raise EngineLimitError(f"the MAP tree has more than {MAX_MAP_NODES} nodes (at least {total}: a missing node that "
                                   f"is not a leaf is the root of a full subtree down to depth {D}); bayesml_amd does not "
                                   f"build it")

    def theta(node, beta):
        if np.all(beta > 1):
            node.theta_vec[:] = (beta - 1) / (np.sum(beta) - k)
        else:
            warnings.warn("MAP estimate of theta_vec doesn't exist for the current h_beta_vec.", ResultWarning)
            node.theta_vec = None

    def full(d, by_rule):
        """A missing node and, unless it is a leaf, the full subtree below it."""
        node = node_cls(d, k)
        node.h_g = hn_g if d < D or by_rule else 0.0
        node.h_beta_vec[:] = model.hn_beta_vec
        theta(node, model.hn_beta_vec)
        return node

    root = None
    stack = [(0, 0, None, 0)]
    while stack:
        d, s, parent, c = stack.pop()
        g, beta, is_leaf = nd[(d, s)]
        node = node_cls(d, k)
        node.h_g = g
        node.h_beta_vec[:] = beta
        theta(node, beta)
        if parent is None:
            root = node
        else:
            parent.children[c] = node
        if is_leaf:
            node.leaf = True
            continue
        for c in range(k):
            cs = _ctsp.child_key(s, d, c, k, D)
            if (d + 1, cs) in nd:
                stack.append((d + 1, cs, node, c))
                continue
            # (ref:755-762: a missing child that its parent's rule makes a leaf keeps hn_g even at the maximal depth)
            rule = 1.0 - g > g * _subtree_pow(hn_g, k, D, d)
            child = full(d + 1, d + 1 == D and rule)
            node.children[c] = child
            if d + 1 == D or rule:
                child.leaf = True
                continue
            below = [child]
            while below:            # the full subtree, level by level (its size was bounded above)
                top = below.pop()
                for cc in range(k):
                    sub = full(top.depth + 1, False)
                    top.children[cc] = sub
                    if sub.depth == D:
                        sub.leaf = True
                    else:
                        below.append(sub)
    return root
