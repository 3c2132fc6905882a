"""The HMM predictive of many sequences on the MI355X (include/hmmbatch.h) against the exact oracle of the single-sequence
pass (tests/hmmpred_oracle.py), sequence by sequence, from what the engine was handed (``HmmBatchPass.last``): the oracle's
bound holds for any summation order of the dot products, so it covers the MFMA recursion unchanged.  Required of every
sequence: |ln p - exact| <= 2 B_t, z equal wherever the oracle decides it, the last phi within a relative 2 H, and
|tot - sum_t ln p_t| <= sum_t 2 B_t + len 2^-52 sum_t |ln p_t|."""
import numpy as np
import pytest
import torch

import contexttree_oracle as orc
import hmmpred_cases as cases
import hmmpred_oracle as ho
from test_hmmpred import hmm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def lengths_of(S, longest=40):
    """S lengths with 0, 1 and 2 among them, unequal inside every sheaf, an empty sequence first and last and the longest
    the last that has rows."""
    if S == 1:
        return np.array([7])
    n = np.array([(3 * i) % 7 for i in range(S)])
    n[:3] = (0, 1, 2)
    n[-1], n[-2] = 0, longest
    return n


def held(label, last, x, off, lnp, z, state, tot):
    """Every sequence to its own oracle."""
    mp = orc._mp()
    g = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)      # noqa: E731
    a, w0, u, mu, nu, pivot = (g(last[k]) for k in ("a", "w0", "u", "mu", "nu", "pivot"))
    x = g(x)
    lnp, z, state, tot = g(lnp), g(z), g(state), g(tot)
    worst = 0.0
    for n in range(len(off) - 1):
        lo, hi = int(off[n]), int(off[n + 1])
        w = w0[n] if w0.ndim == 2 else w0
        if hi == lo:
            assert np.array_equal(state[n], w) and tot[n] == 0.0, (label, n)
            continue
        o = ho.exact(a, w, u, mu, nu, pivot, x[lo:hi])
        r, at = o.ratio(lnp[lo:hi])
        worst = max(worst, r)
        assert r <= 2.0, (label, n, at, r)
        decided = o.z_decided()
        assert np.array_equal(z[lo:hi][decided], o.z[decided]), (label, n)
        assert o.end_ratio(state[n], factor=2) <= 1.0, (label, n)
        err = float(abs(mp.mpf(float(tot[n])) - mp.fsum(o.lnp_mp)))
        assert err <= 2.0 * o.B.sum() + (hi - lo) * ho.EPS * np.abs(o.lnp).sum(), (label, n, err)
    print(f"{label}: worst |error| / B_t = {worst:.3f}")


def engine_run(c, lens, want_tot=True, **kw):
    from bayesml_amd import _hmmbatch
    K, D = c["mu"].shape
    eng = _hmmbatch.HmmBatchPass(K, D, DEV)
    off = np.concatenate([[0], np.cumsum(lens)])
    x = kw.pop("x", c["x"][:off[-1]])
    out = eng.run(torch.as_tensor(x).to(DEV), off, c["a"], kw.pop("w0", c["w0"]), c["mu"], c["nu"], c["u"], True, want_tot, **kw)
    torch.cuda.synchronize()
    return eng, off, out


# ---- 1. sheaf and tile edges, through the model ---------------------------------------------------------------------------------
EDGES = [(1, 15, "f64", "initial"), (3, 1, "f32", "vector"), (16, 16, "strided", "matrix"), (17, 17, "f32", "matrix"),
         (17, 33, "f64", "initial"), (33, 33, "f64", "vector"), (64, 17, "f64", "matrix"), (64, 33, "f32", "initial")]


def model_case(K, S, kind, start):
    m, lens = hmm(K, 3, seed=K + S), lengths_of(S)
    rng = np.random.default_rng([K, S])
    x = (m.hn_m_vecs[rng.integers(0, K, lens.sum())] + rng.standard_normal((lens.sum(), 3))).astype(np.float32 if kind == "f32" else np.float64)
    if kind == "strided":
        wide = torch.zeros(len(x), 5, dtype=torch.float64, device=DEV)
        wide[:, :3] = torch.from_numpy(x).to(DEV)
        x = wide[:, :3]
    w = rng.uniform(0.5, 1.5, (S, K))
    w[:, 0] = np.where(np.arange(S) % 3 == 0, 0.0, w[:, 0]) if K > 1 else w[:, 0]      # (zero entries in some start rows)
    w /= w.sum(axis=1, keepdims=True)
    return m, lens, x, {"initial": "initial", "vector": w[0], "matrix": w}[start]


@pytest.mark.parametrize("K, S, kind, start", EDGES)
def test_sheaf_and_tile_edges(K, S, kind, start):
    m, lens, x, w = model_case(K, S, kind, start)
    lnp, z, state, tot = m.calc_pred_logpdf(x, lengths=lens, start=w, assign=True, return_state=True, totals=True)
    assert lnp.shape == z.shape == (lens.sum(),) and state.shape == (S, K) and tot.shape == (S,)
    assert isinstance(lnp, torch.Tensor) == (kind == "strided")
    eng = m._hmmbatch_pass
    assert any(not np.array_equal(o, np.arange(len(o))) for o in eng.last["order"]) or S == 1      # (a real permutation)
    held(f"K={K} S={S} {kind} {start}", eng.last, x, eng.last["off"], lnp, z, state, tot)


# ---- 6. cuts --------------------------------------------------------------------------------------------------------------------
def test_cuts_at_sequence_boundaries_give_the_same_bits():
    from bayesml_amd import _hmmbatch
    m, lens, x, w = model_case(17, 33, "f64", "matrix")
    kw = dict(lengths=lens, start=w, assign=True, return_state=True, totals=True)
    whole = m.calc_pred_logpdf(x, **kw)
    cut = m.calc_pred_logpdf(x, chunk_bytes=8 * _hmmbatch.scratch_len(17, 3, 64), **kw)
    segs = m._hmmbatch_pass.last["segments"]
    assert len(segs) >= 3 and all(kind == "batch" for kind, _, _ in segs)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(whole, cut))


# ---- 2., 3. the wide path and the plain emission --------------------------------------------------------------------------------
@pytest.mark.parametrize("K, D, band, lens", [(65, 3, None, (0, 5, 12)), (256, 3, 3, (0, 5, 12)), (2, 130, None, (3, 4))])
def test_wide_path_and_plain_emission(K, D, band, lens):
    c = cases.make(K, D, sum(lens), 400 + K, band=band)
    w = np.random.default_rng(K).uniform(0.5, 1.5, (len(lens), K))
    eng, off, out = engine_run(c, lens, w0=w / w.sum(axis=1, keepdims=True))
    held(f"K={K} D={D}", eng.last, c["x"], off, *out)


# ---- 4. batch composition does not enter ----------------------------------------------------------------------------------------
def test_a_sequence_depends_on_no_other():
    lens = lengths_of(20, longest=11)
    c = cases.make(17, 3, int(lens.sum()), 404)
    off = np.concatenate([[0], np.cumsum(lens)])
    w = np.random.default_rng(4).uniform(0.5, 1.5, (20, 17))
    w /= w.sum(axis=1, keepdims=True)
    _, _, (lnp, z, end, _) = engine_run(c, lens, w0=w, pivot=c["x"][5])
    _, _, again = engine_run(c, lens, w0=w, pivot=c["x"][5])
    assert all(torch.equal(u, v) for u, v in zip((lnp, z, end), again))
    rev = np.concatenate([c["x"][off[n]:off[n + 1]] for n in reversed(range(20))])
    _, roff, (rlnp, rz, rend, _) = engine_run(c, lens[::-1], x=rev, w0=w[::-1].copy(), pivot=c["x"][5])
    for n in range(20):
        lo, hi, rlo, rhi = off[n], off[n + 1], roff[19 - n], roff[20 - n]
        assert torch.equal(lnp[lo:hi], rlnp[rlo:rhi]) and torch.equal(z[lo:hi], rz[rlo:rhi]) and torch.equal(end[n], rend[19 - n])


# ---- 5. routing -----------------------------------------------------------------------------------------------------------------
def test_long_sequences_go_through_the_single_sequence_filter():
    from bayesml_amd import _hmmpred
    lens = (7, 4096, 0, 9)
    c = cases.make(4, 2, sum(lens), 405)
    w = np.random.default_rng(5).uniform(0.5, 1.5, (4, 4))
    w /= w.sum(axis=1, keepdims=True)
    eng, off, (lnp, z, end, tot) = engine_run(c, lens, w0=w)
    assert [kind for kind, _, _ in eng.last["segments"]] == ["batch", "single", "batch"]
    one = _hmmpred.HmmFilterPass(4, 2, DEV)
    want = one.run(torch.from_numpy(c["x"][7:4103]).to(DEV), c["a"], w[1], c["mu"], c["nu"], c["u"], True, pivot=eng.last["pivot"])
    assert torch.equal(lnp[7:4103], want[0]) and torch.equal(z[7:4103], want[1]) and torch.equal(end[1], want[2])
    held("routing", eng.last, c["x"], off, lnp, z, end, tot)
