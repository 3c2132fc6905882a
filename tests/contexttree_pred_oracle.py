"""Oracles for ``contexttree.LearnModel.calc_pred_logpdf`` (TEST INFRASTRUCTURE ONLY).

(a) ``pred_rows``: the reference's recursion (bayesml/contexttree/_contexttree.py:954-989) restated in NumPy for every
    position of a held-out sample, with ``lengths``: walk the path of the context to depth e = min(i - start, D), p =
    beta / sum(beta) at its end, then p = (1 - g) * beta / sum(beta) + g * p bottom-up; a node that is not there reads the
    defaults (g = 0 at depth D).  The tree is read through a lookup, ``dense_lookup`` on the tables of ``contexttree_oracle``
    or ``sparse_lookup`` on the node dictionaries of ``contexttree_sparse_oracle``.
(b) ``pred_rows_exact``: the same in mpmath at ``orc.MP_DPS`` digits, binary64 entries taken as exact.
(c) ``CpuPredPass`` / ``use_cpu``: (a) behind the private ``_ctpred_pass_factory`` seam, so that the host logic of the method
    can be tested without a GPU.

The tolerance.  With u = 2**-53: own = beta[a] / sum(beta) has relative error <= (k + 1) u whatever the order in which the
k positive terms are summed ((k - 1) u for the sum, u for the division, u to spare).  One Horner step on non-negative terms,
(1 - g) * b / s + g * p, adds at most 4 u (the subtraction, the product, the division already counted in own, the product
g * p, the sum; non-negative terms cannot cancel).  A path has at most D + 1 nodes, so the computed p is within
``p_rel(k, D)`` = (k + 4 D + 6) u of the exact one, relative, to first order - in the engine and in the reference's binary64
arithmetic alike.  Against the exact value the tests allow twice that (the first-order bound with its second-order terms
covered), plus 2 u max(1, |ln p|) for a logarithm; against the reference's fixture values the sum of both sides' bounds.
"""
import numpy as np
import torch

import contexttree_oracle as orc
import contexttree_sparse_oracle as sorc

U = 2.0 ** -53


# ---- the tolerance -----------------------------------------------------------------------------------------------------------
def p_rel(k, D):
    """First-order relative error of a computed p against the exact one."""
    return (k + 4 * D + 6) * U


def p_rel_exact(k, D):
    """Allowed relative error of a computed p against the mpmath value."""
    return 2 * p_rel(k, D)


def lnp_abs_exact(k, D, lnp):
    """Allowed absolute error of a computed ln p against the mpmath value."""
    return p_rel_exact(k, D) + 2 * U * np.maximum(1.0, np.abs(lnp))


def p_rel_reference(k, D):
    """Allowed relative error of a computed p against the reference's binary64 p: both sides' bounds."""
    return 2 * p_rel_exact(k, D)


def lnp_abs_reference(k, D, lnp):
    """Allowed absolute error of a computed ln p against the logarithm of the reference's binary64 p (taken in binary64
    by the test: its own rounding is inside the logarithm's allowance)."""
    return p_rel_reference(k, D) + 4 * U * np.maximum(1.0, np.abs(lnp))


# ---- lookups -----------------------------------------------------------------------------------------------------------------
def dense_lookup(t, k, D):
    """``get(ctx) -> (g, beta) or None`` on dense tables; ``ctx`` = (x[i-1], ..., x[i-d])."""
    off = orc.offsets(k, D)

    def get(ctx):
        i = off[len(ctx)] + sum(int(c) * k ** j for j, c in enumerate(ctx))
        return (float(t["g"][i]), t["beta"][i]) if t["exists"][i] else None
    return get


def sparse_lookup(nodes, k, D):
    """The same on a node dictionary ``{(level, key): [g, beta, leaf]}``."""
    def get(ctx):
        row = nodes.get((len(ctx), sorc.pack(ctx, k, D)))
        return None if row is None else (float(row[0]), np.asarray(row[1], dtype=float))
    return get


def no_tree(ctx):
    return None


def leave_depth(y, lengths, D, get, i):
    """The depth of the first node missing on the path of position i, or None when the whole path is there."""
    start = starts_of(len(y), lengths)
    for d in range(int(min(i - start[i], D)) + 1):
        if get(tuple(int(v) for v in y[i - d:i][::-1])) is None:
            return d
    return None


def starts_of(n, lengths):
    """The start of the sequence that holds each position."""
    if lengths is None:
        return np.zeros(n, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.sum() == n and np.all(lengths >= 0)
    return np.repeat(np.cumsum(lengths) - lengths, lengths)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def pred_rows(y, lengths, k, D, get, hn_g, hn_beta_vec, only=None):
    """float64 [n, k]: the predictive vector of every position (of the positions ``only``; the other rows stay 0)."""
    y = np.asarray(y, dtype=np.int64)
    hb = np.asarray(hn_beta_vec, dtype=float)
    start = starts_of(len(y), lengths)
    rows = np.zeros((len(y), k))
    for i in (range(len(y)) if only is None else only):
        e = int(min(i - start[i], D))
        path = []
        for d in range(e + 1):
            node = get(tuple(int(v) for v in y[i - d:i][::-1]))
            path.append(node if node is not None else (0.0 if d == D else float(hn_g), hb))
        p = path[e][1] / path[e][1].sum()
        for d in range(e - 1, -1, -1):
            g, beta = path[d]
            p = (1 - g) * beta / beta.sum() + g * p
        rows[i] = p
    return rows


def outputs(rows, y, lengths):
    """(lnp, z, totals) of the rows: what ``calc_pred_logpdf`` returns beside them."""
    y = np.asarray(y, dtype=np.int64)
    lnp = np.log(rows[np.arange(len(y)), y])
    tot = None
    if lengths is not None:
        at = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
        tot = np.array([lnp[a:b].sum() for a, b in zip(at[:-1], at[1:])])
    return lnp, rows.argmax(1).astype(np.int64), tot


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def pred_rows_exact(y, lengths, k, D, get, hn_g, hn_beta_vec):
    """[n][k] mpf."""
    mp = orc._mp()
    y = [int(v) for v in y]
    hb = [mp.mpf(float(v)) for v in hn_beta_vec]
    start = starts_of(len(y), lengths)
    out = []
    for i in range(len(y)):
        e = int(min(i - start[i], D))
        path = []
        for d in range(e + 1):
            node = get(tuple(y[i - d:i][::-1]))
            if node is None:
                path.append((mp.mpf(0.0 if d == D else float(hn_g)), hb))
            else:
                path.append((mp.mpf(node[0]), [mp.mpf(float(v)) for v in node[1]]))
        s = mp.fsum(path[e][1])
        p = [v / s for v in path[e][1]]
        for d in range(e - 1, -1, -1):
            g, beta = path[d]
            s = mp.fsum(beta)
            p = [(1 - g) * v / s + g * q for v, q in zip(beta, p)]
        out.append(p)
    return out


# ---- the held-out samples of the fixtures, shared by tests/golden/make_golden_contexttree_pred.py and the tests ---------------
def heldout(case, x1):
    """A seeded held-out sample of 3 (D + 2) + 40 symbols and its ``lengths``: sequences of 0, 1, D, D + 1, 0 symbols and
    a long one.  The long one alternates runs copied from the training sample ``x1`` (paths that stay in the tree) with
    uniform runs (paths that leave it)."""
    k, D = case["k"], case["D"]
    rng = np.random.default_rng([case["seed"], 77])
    n = 3 * (D + 2) + 40
    lengths = np.array([0, 1, D, D + 1, 0, n - (2 * D + 2)], dtype=np.int64)
    y = rng.integers(0, k, n).astype(np.int64)
    x1 = np.asarray(x1, dtype=np.int64)
    run = D + 6
    at = int(lengths[:5].sum())
    while at + run <= n and len(x1) >= run:
        src = int(rng.integers(0, len(x1) - run + 1))
        y[at:at + run] = x1[src:src + run]
        at += 2 * run
    return y, lengths


def z_clear(rows, k, D):
    """Positions whose first maximum a perturbation within the bound cannot move: the top two entries differ by more."""
    top = np.sort(rows, axis=1)
    if k == 1:
        return np.ones(len(rows), bool)
    return top[:, -1] - top[:, -2] > 2 * p_rel_reference(k, D) * top[:, -1]


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
class CpuPredPass:
    """``_ctpred.PredPass`` on the CPU stand-in engines: the tree is read through the store's host view."""

    def __init__(self, eng, store):
        self.eng, self.store = eng, store
        self.launch_info = "cpu stand-in"
        self.calls = 0

    def run(self, x, seq_off, has_tree, hn_g, hn_beta_vec, assign=False, dist=False, totals=False):
        store, k, D = self.store, self.store.k, self.store.D
        self.calls += 1
        v = x.to(torch.int64).numpy()
        bad = int(((v < 0) | (v >= k)).sum())
        y = np.where((v < 0) | (v >= k), 0, v)
        view = store.view(self.eng) if has_tree else None

        def get(ctx):
            if view is None:
                return None
            key = 0
            for d, c in enumerate(ctx):
                key = store.child(d, key, int(c))
            if (len(ctx), key) not in view:
                return None
            g, beta, _ = view.get(len(ctx), key)
            return float(g), np.asarray(beta, dtype=float)
        lengths = None if seq_off is None else np.diff(np.asarray(seq_off, dtype=np.int64))
        rows = pred_rows(y, lengths, k, D, get, hn_g, hn_beta_vec)
        lnp, z, tot = outputs(rows, y, lengths)
        t = torch.from_numpy
        return (bad, t(lnp), t(z) if assign else None, t(rows) if dist else None, t(tot) if totals else None)


def use_cpu(model, sparse=False):
    """Route a model through the CPU stand-ins of both seams."""
    from fake_contexttree_engine import CpuCtreePass, CpuSparseCtreePass
    model._ctree_pass_factory = CpuSparseCtreePass if sparse else CpuCtreePass
    model._ctpred_pass_factory = CpuPredPass
    return model
