"""Oracles for ``LearnModel.pred_and_update_sequence`` (TEST INFRASTRUCTURE ONLY).

(a) ``seq_pass``: the level-wise form of DESIGN.md "Sequential prediction" in NumPy on the dense tables of
    ``contexttree_oracle`` - positions sorted by key per level, counts as ranks, a node's log-odds as its start plus a
    segmented prefix sum.  ``CpuSequencePass`` / ``use_cpu`` put it behind the private ``_ctseq_pass_factory`` seam so
    that the host logic of the method can be tested without a GPU.
(b) ``sequence_exact``: the sequential recursion of the reference (bayesml/contexttree/_contexttree.py:1016-1038) in mpmath
    at ``orc.MP_DPS`` digits.
"""
import numpy as np
import torch

import contexttree_oracle as orc
from fake_contexttree_engine import CpuCtreePass


def _sigmoid(L):
    e = np.exp(-np.abs(L))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(L >= 0, big, small), np.where(L >= 0, small, big)


def _run_starts(keys):
    """For ascending ``keys``: the index at which each element's run of equal keys starts."""
    n = len(keys)
    flag = np.ones(n, bool)
    flag[1:] = keys[1:] != keys[:-1]
    return np.maximum.accumulate(np.where(flag, np.arange(n), 0)), flag


def seq_pass(x, begin, m, k, D, t, hn_g, hn_beta_vec, want_rows=True):
    """Positions begin .. begin + m - 1 of ``x`` on the tables ``t`` (updated in place).  Returns (rows [m, k] or None,
    q [m]): the predictive distributions and the probability each gave its own symbol."""
    x = np.asarray(x, dtype=np.int64)
    hb = np.asarray(hn_beta_vec, dtype=float)
    off = orc.offsets(k, D)
    gi = begin + np.arange(m)
    q = np.zeros(m)
    rows = np.zeros((m, k)) if want_rows else None
    for d in range(D, -1, -1):
        pos = np.flatnonzero(gi >= d)
        if not len(pos):
            continue
        key = np.zeros(len(pos), dtype=np.int64)
        for j in range(1, d + 1):
            key += x[gi[pos] - j] * k ** (j - 1)
        order = np.argsort(key, kind="stable")
        pos, key = pos[order], key[order]
        a = x[gi[pos]]
        md = len(pos)
        segst, flag = _run_starts(key)
        heads = np.flatnonzero(flag)
        ends = np.append(heads[1:], md) - 1
        r = np.arange(md) - segst
        node = off[d] + key
        ex = t["exists"][node] != 0
        b0a = np.where(ex, t["beta"][node, a], hb[a])
        sum_head = np.array([t["beta"][node[h]].sum() if ex[h] else hb.sum() for h in heads])
        sumb0 = sum_head[np.cumsum(flag) - 1]
        g0 = np.where(ex, t["g"][node], 0.0 if d == D else hn_g)
        # rank inside the run of (symbol, key)
        order2 = np.argsort(a * k ** d + key, kind="stable")
        rs, _ = _run_starts((a * k ** d + key)[order2])
        ca = np.zeros(md, dtype=np.int64)
        ca[order2] = np.arange(md) - rs
        own = (b0a + ca) / (sumb0 + r)
        end = (gi[pos] == d) | (d == D)
        delta = np.zeros(md)
        delta[~end] = np.log(q[pos][~end]) - np.log(own[~end])
        excl = np.zeros(md)
        for h, e in zip(heads, ends):
            if e > h:
                excl[h + 1:e + 1] = np.cumsum(delta[h:e])
        fixed = ~((g0 > 0) & (g0 < 1))
        g, omg = g0.copy(), 1.0 - g0
        free = ~fixed
        L0 = np.zeros(md)
        L0[free] = np.log(g0[free]) - np.log1p(-g0[free])
        later = free & (r > 0)
        g[later], omg[later] = _sigmoid(L0[later] + excl[later])
        q[pos] = np.where(end, own, omg * own + g * q[pos])
        if want_rows:
            onehot = np.zeros((md, k), dtype=np.int64)
            onehot[np.arange(md), a] = 1
            before = np.cumsum(onehot, axis=0) - onehot
            before -= before[segst]
            B0 = np.where(ex[:, None], t["beta"][node], hb[None, :])
            own_rows = (B0 + before) / (sumb0 + r)[:, None]
            rows[pos] = np.where(end[:, None], own_rows, (1.0 - g)[:, None] * own_rows + g[:, None] * rows[pos])
        # the tables after the chunk
        gout = g0[ends].copy()
        move = free[ends] & (d < D) & ~(end[ends] & (r[ends] == 0))
        gout[move] = _sigmoid(L0[ends][move] + excl[ends][move] + delta[ends][move])[0]
        hn, new = node[heads], ~ex[heads]
        t["beta"][hn[new]] = hb
        t["leaf"][hn[new]] = 1 if d == D else 0
        t["exists"][hn] = 1
        t["g"][hn] = gout
        cnt = np.zeros((len(heads), k), dtype=np.int64)
        np.add.at(cnt, (np.cumsum(flag) - 1, a), 1)
        t["beta"][hn] = np.where(cnt > 0, t["beta"][hn] + cnt, t["beta"][hn])
    return rows, q


def sequence(x, k, D, t, hn_g, hn_beta_vec, m=None, want_rows=True):
    """The whole sample in chunks of ``m`` (default: one chunk).  Returns (rows or None, nats)."""
    n = len(x)
    m = n if m is None else m
    out = [seq_pass(x, b, min(m, n - b), k, D, t, hn_g, hn_beta_vec, want_rows) for b in range(0, n, m)]
    rows = np.concatenate([o[0] for o in out]) if want_rows else None
    return rows, -np.log(np.concatenate([o[1] for o in out]))


# ---- the CPU engines behind the model's two seams -----------------------------------------------------------------------
class CpuCtreePassSeq(CpuCtreePass):
    """``CpuCtreePass`` with ``CtreePass.count``'s [n | bad] head."""

    def count(self, x):
        v = x.to(torch.int64)
        return torch.tensor([v.shape[0], int(((v < 0) | (v >= self.k)).sum())], dtype=torch.int64)


class CpuSequencePass:
    def __init__(self, eng):
        self.eng = eng
        self.launch_info = ""
        self.passes = 0

    def run(self, x, hn_g, hn_beta_vec, want, want_nats, chunk_bytes=None):
        from bayesml_amd import _ctseq
        eng = self.eng
        v = x.to(torch.int64).numpy()
        m = _ctseq.plan_chunks(len(v), eng.k, eng.D, want == "argmax", chunk_bytes)
        rows, nats = sequence(v, eng.k, eng.D, eng.t, hn_g, hn_beta_vec, m, want is not None)
        self.passes = -(-len(v) // m)
        self.launch_info = f"cpu stand-in x {self.passes} (m = {m})"
        pred = None
        if want == "rows":
            pred = torch.from_numpy(rows)
        elif want == "argmax":
            pred = torch.from_numpy(rows.argmax(1))
        return pred, torch.from_numpy(nats) if want_nats else None, None if rows is None else torch.from_numpy(rows[-1])


def use_cpu(cls_or_model):
    is_cls = isinstance(cls_or_model, type)
    cls_or_model._ctree_pass_factory = staticmethod(CpuCtreePassSeq) if is_cls else CpuCtreePassSeq
    cls_or_model._ctseq_pass_factory = staticmethod(CpuSequencePass) if is_cls else CpuSequencePass
    return cls_or_model


# ---- (b) the exact recursion --------------------------------------------------------------------------------------------
def sequence_exact(x, k, D, t, hn_g, hn_beta_vec):
    """n steps of the reference's ``pred_and_update`` in mpmath from the tables ``t`` (not modified; binary64 entries taken
    as exact).  Returns a dict:
    ``p``       [n][k] mpf, the exact p_0(i);
    ``p_bound`` [n] mpf: sum over the path of position i of g_bound(g_d, B_d) before the visit, the first-order image in a
                row of log-odds errors of 64 eps B per node (the mixture weights and the rows below are <= 1);
    ``g``, ``logit``, ``B``, ``exists``: per node after the sample - the exact h_g, the exact log-odds where 0 < g < 1 (else
                None) and B = |logit g0| + sum over the node's visits of (|ln p_below[a]| + |ln own[a]|), the size of the
                terms that entered its log-odds."""
    mp = orc._mp()
    off = orc.offsets(k, D)
    hb = [mp.mpf(float(v)) for v in hn_beta_vec]
    nodes = {}

    def node_of(d, key):
        i = off[d] + key
        if i not in nodes:
            if t["exists"][i]:
                b, g = [mp.mpf(float(v)) for v in t["beta"][i]], mp.mpf(float(t["g"][i]))
            else:
                b, g = list(hb), mp.mpf(0.0 if d == D else float(hn_g))
            free = 0 < g < 1
            L = mp.log(g) - mp.log1p(-g) if free else None
            nodes[i] = dict(b=b, g=g, L=L, B=abs(L) if free else mp.mpf(0))
        return nodes[i]

    x = [int(v) for v in x]
    P, bounds = [], []
    for i, a in enumerate(x):
        e = min(i, D)
        path, key = [], 0
        for d in range(e + 1):
            if d > 0:
                key += x[i - d] * k ** (d - 1)
            path.append(node_of(d, key))
        bound = mp.fsum(orc.g_bound(nd["g"], float(nd["B"])) for nd in path[:-1]) if e > 0 else mp.mpf(0)
        nd = path[e]
        sb = mp.fsum(nd["b"])
        p = [v / sb for v in nd["b"]]
        nd["b"][a] += 1
        for d in range(e - 1, -1, -1):
            nd = path[d]
            sb = mp.fsum(nd["b"])
            own = [v / sb for v in nd["b"]]
            nd["b"][a] += 1
            g = nd["g"]
            mixed = [(1 - g) * o + g * pb for o, pb in zip(own, p)]
            if nd["L"] is not None:
                nd["L"] += mp.log(p[a]) - mp.log(own[a])
                nd["B"] += abs(mp.log(p[a])) + abs(mp.log(own[a]))
                nd["g"] = g * p[a] / mixed[a]
            p = mixed
        P.append(p)
        bounds.append(bound)
    n_nodes = off[-1]
    out = dict(p=P, p_bound=bounds, g=np.full(n_nodes, None, dtype=object), logit=np.full(n_nodes, None, dtype=object),
               B=np.zeros(n_nodes), exists=np.array(t["exists"], dtype=np.uint8).copy())
    for i, nd in nodes.items():
        out["g"][i], out["logit"][i], out["B"][i], out["exists"][i] = nd["g"], nd["L"], float(nd["B"]), 1
    return out
