"""The host side of ``contexttree.LearnModel``'s node tree, written once for both storages.

A **store** is chosen once per model from ``tables`` and knows its storage: the limit, the engine, how the tables are saved
and restored, the key arithmetic of a level and the address of a node in the form the engine's own ``gather`` / ``scatter``
take (``_ctree.CtreePass``: a flat table index; ``_ctsp.SparseCtreePass``: ``(level, key)``).  A **view** is a host snapshot
of the node set, addressed by ``(level, key)`` on both sides; the dense key is the index within the level.  The dense view
wraps the NumPy tables of ``get_tables()`` and answers by ``off[level] + key`` without an object per node; the sparse view
wraps a dict of the rows of ``get_nodes()``.  ``hn_root``, ``set_hn_root``, ``path`` and ``map_tree`` below are the model's
tree algorithms on a view; each is called from the method of ``LearnModel`` it serves, with the model as first argument.
"""
import warnings

import numpy as np

from .. import _ctree, _ctsp
from .._engine import EngineLimitError
from .._exceptions import ResultWarning


# ---- views -----------------------------------------------------------------------------------------------------------------
class _View:
    """What both views share.  ``child`` / ``above`` are the store's key arithmetic: ``above(d, s)`` is the parent's key p
    and the symbol c with ``child(d - 1, p, c) == s``.  ``ml`` holds the engine's MAP flags by address, where asked for."""

    def __init__(self, store, ml):
        self.store, self.ml, self.child, self.above = store, ml, store.child, store.above

    def create(self, d, s):
        self.set(d, s, 0.5, np.full(self.store.k, 0.5), 0)

    def map_leaf(self, d, s):
        return bool(self.ml[self.store.address(d, s)])


class _DenseView(_View):
    def __init__(self, store, t, ml=None):
        super().__init__(store, ml)
        self.t = t

    def __contains__(self, at):
        return bool(self.t["exists"][self.store.address(*at)])

    def __iter__(self):
        """Canonical order: level, then key."""
        off = self.store.off
        for d in range(self.store.D + 1):
            for s in np.flatnonzero(self.t["exists"][off[d]:off[d + 1]]):
                yield d, int(s)

    def get(self, d, s):
        i = self.store.address(d, s)
        return float(self.t["g"][i]), self.t["beta"][i], int(self.t["leaf"][i])

    def set(self, d, s, g, beta, leaf):
        i = self.store.address(d, s)
        self.t["exists"][i], self.t["g"][i], self.t["beta"][i], self.t["leaf"][i] = 1, g, beta, leaf

    def reset_below(self, roots, g_of_depth, beta):
        """The None-branch of ref:547-576: the defaults to every existing node at and below each of ``roots``."""
        k, D, off, t = self.store.k, self.store.D, self.store.off, self.t
        for d, s in roots:
            for dd in range(d, D + 1):
                idx = off[dd] + s + k ** d * np.arange(k ** (dd - d))
                idx = idx[t["exists"][idx] != 0]
                t["g"][idx] = g_of_depth(dd)
                t["beta"][idx] = beta

    def saved(self):
        return self.t


class _SparseView(_View):
    def __init__(self, store, nodes, ml=None):
        self.nd = {(int(d), int(s)): [float(g), b, int(lf)]
                   for d, s, g, b, lf in zip(nodes["level"], nodes["key"], nodes["g"], nodes["beta"], nodes["leaf"])}
        super().__init__(store, None if ml is None else dict(zip(self.nd, ml)))     # (both in the canonical order)

    def __contains__(self, at):
        return at in self.nd

    def __iter__(self):
        return iter(sorted(self.nd))

    def get(self, d, s):
        return self.nd[(d, s)]

    def set(self, d, s, g, beta, leaf):
        self.nd[(d, s)] = [float(g), np.array(beta, dtype=float), int(leaf)]

    def reset_below(self, roots, g_of_depth, beta):
        """As ``_DenseView.reset_below``, in one scan of the nodes however many roots there are."""
        roots, b, D = set(roots), self.store.b, self.store.D
        keep = {d: ~((1 << (b * (D - d))) - 1) for d, _ in roots}      # the key bits of the levels 1..d
        for (dd, ss), row in self.nd.items():
            if any(d <= dd and (d, ss & m) in roots for d, m in keep.items()):
                row[0], row[1] = g_of_depth(dd), np.array(beta, dtype=float)

    def saved(self):
        """``get_nodes`` arrays, in canonical order."""
        order, nd = sorted(self.nd), self.nd
        return dict(level=np.array([d for d, _ in order], dtype=np.int32), key=np.array([s for _, s in order], dtype=np.int64),
                    g=np.array([nd[i][0] for i in order], dtype=np.float64),
                    beta=np.array([nd[i][1] for i in order], dtype=np.float64).reshape(len(order), self.store.k),
                    leaf=np.array([nd[i][2] for i in order], dtype=np.uint8))


# ---- stores ----------------------------------------------------------------------------------------------------------------
class _Store:
    sparse, off = False, None
    max_map_nodes = None              # estimate_params builds no MAP tree of more nodes (None: no cap)

    def __init__(self, k, D):
        self.check_limit(k, D)
        self.k, self.D = k, D

    def make_engine(self, model):
        make = model._ctree_pass_factory
        return make(self.k, self.D) if make is not None else self.engine_cls(self.k, self.D, model._device)

    def view(self, eng, map_leaf=False, hn_g=None):
        """A host snapshot of the nodes; with ``map_leaf`` also of the engine's MAP flags under ``hn_g``."""
        ml = eng.map_leaf(hn_g) if map_leaf else None
        return self.view_cls(self, self.save(eng), ml)

    def commit(self, eng, view):
        self.restore(eng, view.saved())


class DenseStore(_Store):
    """``_ctree.CtreePass``: level d starts at ``off[d]``; the key of (x[i-1], ..., x[i-d]) is ``sum_j x[i-j] k^(j-1)``."""
    engine_cls, view_cls = _ctree.CtreePass, _DenseView
    check_limit = staticmethod(_ctree.check_limit)

    def __init__(self, k, D):
        super().__init__(k, D)
        self.off = _ctree.offsets(k, D)

    def address(self, d, s):
        return self.off[d] + s

    def child(self, d, s, c):
        return s + c * self.k ** d

    def above(self, d, s):
        return s % self.k ** (d - 1), s // self.k ** (d - 1)

    def save(self, eng):
        return eng.get_tables()

    def restore(self, eng, saved):
        eng.set_tables(saved)

    def pred_tables(self, eng):
        """What ``_ctpred.PredPass`` reads: the device tensors and the first slot of every level."""
        return dict(beta=eng.beta, g=eng.g, exists=eng.exists, off=self.off)


class SparseStore(_Store):
    """``_ctsp.SparseCtreePass``: the key packs the context, ``_ctsp.symbol_bits(k)`` bits per symbol from the top."""
    sparse = True
    engine_cls, view_cls = _ctsp.SparseCtreePass, _SparseView
    check_limit = staticmethod(_ctsp.check_limit)
    # a missing node under hn_g = 1 is the root of a full subtree of (k^(D-d+1) - 1) / (k - 1) nodes; the count is taken
    # before a single node is built
    max_map_nodes = 1 << 20

    def __init__(self, k, D):
        super().__init__(k, D)
        self.b = _ctsp.symbol_bits(k)

    def address(self, d, s):
        return (d, s)

    def child(self, d, s, c):
        return _ctsp.child_key(s, d, c, self.k, self.D)

    def above(self, d, s):
        return _ctsp.parent_key(s, d, self.k, self.D), (s >> (self.b * (self.D - d))) & ((1 << self.b) - 1)

    def save(self, eng):
        return eng.get_nodes()

    def restore(self, eng, saved):
        eng.set_nodes(saved)

    def pred_tables(self, eng):
        """As ``DenseStore.pred_tables``, with the keys; ``off`` holds the capacities as they are now."""
        return dict(beta=eng.beta, g=eng.g, exists=eng.exists, off=list(eng.off), key=eng.key)


def store_for(sparse, k, D):
    return (SparseStore if sparse else DenseStore)(k, D)


# ---- the model's tree algorithms, on a view --------------------------------------------------------------------------------
def hn_root(model, node_cls):
    """The posterior as the reference's ``_Node`` tree, children in symbol order."""
    view = model._store.view(model._eng())
    made = {}
    for d, s in view:
        g, beta, leaf = view.get(d, s)
        made[(d, s)] = node = node_cls(d, model.c_k, g)
        node.h_beta_vec[:] = beta
        node.leaf = bool(leaf)
        if d > 0:
            p, c = view.above(d, s)
            made[(d - 1, p)].children[c] = node
    return made[(0, 0)]


def set_hn_root(model, root):
    """ref:547-576: superpose the tree ``root`` on the posterior (on a lone default root where there is none)."""
    eng, store, k, D = model._eng(), model._store, model.c_k, model.c_d_max
    if not model._has_root:
        eng.clear()
    view = store.view(eng)
    if not model._has_root:
        view.create(0, 0)
    # (an explicit stack: a tree may be 63 levels deep.  Where ``root`` ends, everything below gets the defaults; those
    # subtrees are disjoint from every node written here, so they are collected and reset in one go.)
    ended, stack = [], [(0, 0, root)]
    while stack:
        d, s, orig = stack.pop()
        if orig is None:
            ended.append((d, s))
        elif d == D or orig.leaf:
            view.set(d, s, 0.0 if d == D else orig.h_g, orig.h_beta_vec, 1)
        else:
            view.set(d, s, orig.h_g, orig.h_beta_vec, 0)
            for c in range(k):
                cs = view.child(d, s, c)
                if (d + 1, cs) not in view:
                    view.create(d + 1, cs)
                stack.append((d + 1, cs, orig.children[c]))
    view.reset_below(ended, model._default_g, model.hn_beta_vec)
    store.commit(eng, view)
    model._has_root = True


def path(model, x):
    """The D + 1 (or fewer) nodes that the context before x[-1] selects, missing ones with the defaults as ref:956-965.
    Returns (addresses, g, beta, leaf)."""
    store, D = model._store, model.c_d_max
    i = x.shape[0] - 1
    depth = min(i, D)
    at, key = [store.address(0, 0)], 0
    for d in range(depth):
        key = store.child(d, key, int(x[i - d - 1]))
        at.append(store.address(d + 1, key))
    g, beta, exists, leaf = model._eng().gather(at)
    g, beta, leaf = g.copy(), beta.copy(), leaf.copy()
    for d in range(depth + 1):
        if not exists[d]:
            g[d], beta[d], leaf[d] = model._default_g(d), model.hn_beta_vec, d == D
    return at, g, beta, leaf


def _subtree_pow(hn_g, k, D, depth):
    """The reference's price of a full subtree under a missing child of a node at ``depth`` (ref:757); k = 1 takes the
    limit D - depth of the geometric sum."""
    m = (k ** (D - depth) - 1) / (k - 1) if k > 1 else float(D - depth)
    return hn_g ** (m - 1) if hn_g > 0 or m > 1 else 1.0


def map_tree(model, node_cls):
    """The MAP tree (ref:733-831).  The engine's flags decide the existing nodes; a missing child gets its parent's rule
    here.  Only the pruned tree is built, and where the store caps it, its size is counted first."""
    k, D, hn_g, cap = model.c_k, model.c_d_max, model.hn_g, model._store.max_map_nodes
    view = model._store.view(model._eng(), map_leaf=True, hn_g=hn_g)

    def rule(d, g):
        """Whether the parent's rule makes a missing child of the existing node (depth d, h_g = g) a leaf (ref:755-762)."""
        return 1.0 - g > g * _subtree_pow(hn_g, k, D, d)

    # the size first: existing internal nodes are walked, a missing child is one leaf or one full subtree down to depth D
    total, stack = 0, [(0, 0)] if cap is not None else []
    while stack:
        d, s = stack.pop()
        total += 1
        if view.map_leaf(d, s):
            continue
        g = view.get(d, s)[0]
        for c in range(k):
            cs = view.child(d, s, c)
            if (d + 1, cs) in view:
                stack.append((d + 1, cs))
            elif d + 1 == D or rule(d, g):
                total += 1
            else:
                total += D - d if k == 1 else (k ** (D - d) - 1) // (k - 1)
        if total > cap:
            raise EngineLimitError(f"the MAP tree has more than {cap} nodes (at least {total}: a missing node that "
                                   f"is not a leaf is the root of a full subtree down to depth {D}); bayesml_amd does not "
                                   f"build it")

    def make(d, g, beta, leaf):
        node = node_cls(d, k, g)
        node.h_beta_vec[:] = beta
        node.leaf = leaf
        if np.all(beta > 1):
            node.theta_vec[:] = (beta - 1) / (np.sum(beta) - k)
        else:
            warnings.warn("MAP estimate of theta_vec doesn't exist for the current h_beta_vec.", ResultWarning)
            node.theta_vec = None
        return node

    def missing(d, by_rule):
        """A missing node: a leaf at the maximal depth or by its parent's rule, else the root of a full subtree.
        (ref:755-762: one that the rule makes a leaf keeps hn_g even at the maximal depth)"""
        return make(d, hn_g if d < D or by_rule else 0.0, model.hn_beta_vec, d == D or by_rule)

    root = None
    stack = [(0, 0, None, 0)]
    while stack:
        d, s, parent, c = stack.pop()
        g, beta, _ = view.get(d, s)
        node = make(d, g, beta, view.map_leaf(d, s))
        if parent is None:
            root = node
        else:
            parent.children[c] = node
        if node.leaf:
            continue
        for c in range(k):
            cs = view.child(d, s, c)
            if (d + 1, cs) in view:
                stack.append((d + 1, cs, node, c))
                continue
            node.children[c] = child = missing(d + 1, rule(d, g))
            below = [] if child.leaf else [child]
            while below:            # the full subtree, level by level (its size was bounded above where a cap holds)
                top = below.pop()
                for cc in range(k):
                    top.children[cc] = sub = missing(top.depth + 1, False)
                    if not sub.leaf:
                        below.append(sub)
    return root
