"""``contexttree.LearnModel.update_posterior(x, lengths=...)`` on the MI355X against the reference's loop
``for s in seqs: update_posterior(s)``, restated per symbol (ref:688-731) in mpmath at 50 digits on one tree.

h_beta_vec, exists and leaf are compared bit for bit (the priors are multiples of 1/2, so adding the symbols one by one
is exact).  h_g is held to ``contexttree_oracle.g_bound``, the bound of tests/test_gpu_contexttree_rows.py: a log-odds
error of 64 eps B, where B sums, over the node's subtree, the sizes of the terms that enter a node's log-odds in this
call: row_scale(b0, cnt) + |lead| + |logit g0|.  Its image in g, 64 eps B g (1 - g) + eps g, is what is compared, so that a
g within 1e-9 of 0 or 1 is compared in g.

Shapes: (2, 3) and (3, 2) count in LDS histograms, (4, 6) by global atomics.  ``mixed`` has lengths 0, 1, D - 1, D, D + 1, a
boundary one position before the tile edge at 256 and a sequence across it; ``many`` has more than CTFIT_SEQ_STAGE + 1
sequences that touch the first tile and a root run past CTFIT_SERIAL_RUN.  Every case updates twice, so that the second
call reads b0 and g0 from the tables.
"""
import os

import numpy as np
import pytest
import torch

import contexttree_oracle as orc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def exact_loop(t, x, lengths, k, D, hn_g, hn_beta):
    """The per-symbol loop over every sequence on the tables ``t`` (beta float64, g as mpf objects), in place.  Returns B
    per node for this call."""
    mp = orc._mp()
    off = orc.offsets(k, D)
    b0, g0 = t["beta"].copy(), t["g"].copy()
    lead, inner = np.zeros(off[-1]), np.zeros(off[-1], bool)
    at = 0
    for n in lengths:
        seq = [int(v) for v in x[at:at + n]]
        at += n
        for i, a in enumerate(seq):
            e, key, path = min(i, D), 0, []
            for d in range(e + 1):
                if d > 0:
                    key += seq[i - d] * k ** (d - 1)
                j = off[d] + key
                if not t["exists"][j]:
                    t["exists"][j], t["beta"][j], t["g"][j] = 1, hn_beta, mp.mpf(0.0 if d == D else hn_g)
                    b0[j], g0[j] = hn_beta, t["g"][j]
                    t["leaf"][j] = d == D
                path.append(j)
            p = None
            for d in range(e, -1, -1):
                j = path[d]
                own = mp.mpf(float(t["beta"][j, a])) / mp.mpf(float(t["beta"][j].sum()))
                t["beta"][j, a] += 1.0
                if d == e:
                    p = own
                    if e < D:
                        lead[j] += abs(float(mp.log(own)))
                else:
                    mixed = (1 - t["g"][j]) * own + t["g"][j] * p
                    t["g"][j] = t["g"][j] * p / mixed
                    p, inner[j] = mixed, True
    B = np.zeros(off[-1])
    for d in range(D, -1, -1):
        for s in range(k ** d):
            j = off[d] + s
            cnt = np.rint(t["beta"][j] - b0[j]).astype(np.int64) if t["exists"][j] else np.zeros(k, np.int64)
            if cnt.sum() == 0:
                continue
            B[j] = orc.row_scale(b0[j], cnt) + lead[j]
            if d < D:
                B[j] += sum(B[off[d + 1] + s + c * k ** d] for c in range(k))
                if inner[j] and 0 < g0[j] < 1:
                    B[j] += abs(float(mp.log(g0[j]) - mp.log1p(-g0[j])))
    return B


def mp_tables(k, D):
    t = orc.new_tables(k, D)
    t["g"] = np.array([orc._mp().mpf(0)] * len(t["g"]), dtype=object)
    return t


def hold(got, want, B, label):
    assert np.array_equal(got["exists"], want["exists"]), label
    ex = want["exists"] != 0
    assert np.array_equal(got["leaf"][ex], want["leaf"][ex]), label
    assert np.array_equal(got["beta"][ex], want["beta"][ex]), label
    mp, worst = orc._mp(), (0.0, None)
    for j in np.flatnonzero(ex):
        err = abs(mp.mpf(float(got["g"][j])) - want["g"][j])
        worst = max(worst, (float(err / orc.g_bound(want["g"][j], B[j])), (j, got["g"][j], float(want["g"][j]), B[j])))
    print(f"{label}: err / bound = {worst[0]:.3g}")
    assert worst[0] <= 1.0, (label, worst)


def lengths_of(kind, D):
    if kind == "two":
        return [5, 7]
    if kind == "mixed":
        first = [0, 1, D - 1, D, D + 1]
        return first + [255 - sum(first), 300, 0, 2 * D + 1, 0]
    return [1] * 40 + [0] * 500 + [2] * 30 + [D + 2] * 20 + [0] * 3 + [1]         # "many": 594 sequences in 221 positions


CASES = [(2, 3, "two", np.uint8), (2, 3, "mixed", np.int64), (2, 3, "many", np.int32), (3, 2, "mixed", np.uint8),
         (3, 2, "many", np.int64), (4, 6, "mixed", np.int32), (4, 6, "many", np.uint8)]


@pytest.mark.parametrize("k, D, kind, dtype", CASES, ids=[f"k{c[0]}D{c[1]}-{c[2]}-{np.dtype(c[3]).name}" for c in CASES])
def test_two_batches_against_the_exact_loop(k, D, kind, dtype):
    from bayesml_amd import contexttree
    rng = np.random.default_rng(k * 100 + D)
    lengths = lengths_of(kind, D)
    m = contexttree.LearnModel(k, D, h0_g=0.4, device="cuda:0")
    want, B, before = mp_tables(k, D), 0.0, None
    for call in range(2):
        x = rng.integers(0, k, sum(lengths)).astype(dtype)
        if kind == "many":
            x[:40:2] = x[0]              # the root's run: runs of heads with one symbol between heads with others
        B_call = exact_loop(want, x, lengths, k, D, 0.4, np.full(k, 0.5))
        B = B + B_call                   # (the second call's logit g0 carries the first call's error)
        m.update_posterior(x if call == 0 else torch.from_numpy(x).cuda(), lengths=lengths)
        got = m._engine.get_tables()
        hold(got, want, B, f"call {call}")
        if before is not None:           # a node without visits in this call keeps its bits
            quiet = (B_call == 0) & (before["exists"] != 0)
            assert np.array_equal(got["g"][quiet], before["g"][quiet])
        before, lengths = got, lengths[::-1]


def test_heads_only_leave_h_g_alone():
    from bayesml_amd import contexttree
    k, D = 2, 3
    rng = np.random.default_rng(5)
    m = contexttree.LearnModel(k, D, device="cuda:0").update_posterior(rng.integers(0, k, 50))
    before = m._engine.get_tables()
    m.update_posterior(np.array([0, 1, 0]), lengths=[1, 1, 1, 0])
    after = m._engine.get_tables()
    assert after["g"].tobytes() == before["g"].tobytes()
    assert np.array_equal(after["beta"][0] - before["beta"][0], [2, 1])
    assert np.array_equal(after["beta"][1:], before["beta"][1:])


def test_identities():
    from bayesml_amd import contexttree
    k, D = 3, 2
    x = np.random.default_rng(9).integers(0, k, 40)
    new = lambda: contexttree.LearnModel(k, D, device="cuda:0")                  # noqa: E731
    tabs = lambda mdl: {n: a.tobytes() for n, a in mdl._engine.get_tables().items()}      # noqa: E731
    parent = tabs(new().update_posterior(x))
    assert tabs(new().update_posterior(x, lengths=[40])) == parent
    assert tabs(new().update_posterior(x, lengths=[0, 40, 0])) == parent
    assert tabs(new().update_posterior(x, lengths=[20, 20])) != parent           # no context crosses position 20
    m = new().update_posterior(x, lengths=[20, 20])
    held, hn = tabs(m), (m.hn_g, m.hn_beta_vec.copy())
    bad = x.copy()
    bad[-1] = k
    from bayesml_amd._exceptions import DataFormatError
    with pytest.raises(DataFormatError):
        m.update_posterior(bad, lengths=[5, 35])
    assert tabs(m) == held and m.hn_g == hn[0] and np.array_equal(m.hn_beta_vec, hn[1])


@pytest.mark.parametrize("name", ["contexttree_segments_k2d3", "contexttree_segments_k3d2"])
def test_golden_from_the_reference_loop(name):
    """The reference's own loop, recorded in binary64.  Its side of the bound: every visit multiplies h_g by p / mixed, each
    of which carries the roundings of the D + 1 levels below it, so h_g has a relative error of at most
    4 (D + 1) visits eps; and 1 - h_g the same, because mixed - g p = (1 - g) own is formed without cancellation."""
    from bayesml_amd import contexttree
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    k, D, x, lengths = int(z["k"]), int(z["D"]), z["x"], z["lengths"]
    m = contexttree.LearnModel(k, D, h0_g=float(z["h0_g"]), device="cuda:0").update_posterior(x, lengths=lengths)
    got = m._engine.get_tables()
    want = mp_tables(k, D)
    B = exact_loop(want, x, list(lengths), k, D, float(z["h0_g"]), np.full(k, 0.5))
    assert np.array_equal(got["exists"], z["exists"]) and np.array_equal(got["beta"][z["exists"] != 0], z["beta"][z["exists"] != 0])
    eps = 2.0 ** -52
    for j in np.flatnonzero(z["exists"]):
        g = float(z["g"][j])
        visits = float(z["beta"][j].sum() - 0.5 * k)
        ours = float(orc.g_bound(orc._mp().mpf(g), B[j]))
        theirs = 4 * (D + 1) * visits * eps * min(g, 1 - g)
        assert abs(got["g"][j] - g) <= ours + theirs, (name, j)
