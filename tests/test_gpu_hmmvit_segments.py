"""Viterbi over many sequences laid end to end (csrc/hmmvit_kernels.h) against a plain binary64 recursion per segment.  The
recursion is additions and comparisons in a fixed order, so binary64 in that order is the exact reference: np.array_equal."""
import numpy as np
import pytest
import torch

from oracle import hmm_vb_oracle as orc
from test_gpu_hmmseg import random_posterior

pytestmark = pytest.mark.gpu

# the prefetch depth and the backtrack block on both sides; the first five are the whole batch at G = 1
LENGTHS = [129, 0, 65, 9, 64, 8, 63, 17, 1, 2]


def viterbi_reference(ln_rho, ln_pi, ln_a, off):
    """(z [T], whether any maximum or final arg-max met an exact tie)."""
    z, tie = np.full(ln_rho.shape[0], -1, dtype=np.int32), False
    for lo, hi in ((a, b) for a, b in zip(off[:-1], off[1:]) if b > a):
        omega, phi = ln_rho[lo] + ln_pi, np.zeros((hi - lo, len(ln_pi)), dtype=np.int64)
        for t in range(1, hi - lo):
            cand = omega[:, None] + ln_a
            phi[t], best = cand.argmax(axis=0), cand.max(axis=0)
            tie |= bool(((cand == best).sum(axis=0) > 1).any())
            omega = ln_rho[lo + t] + best
        tie |= bool((omega == omega.max()).sum() > 1)
        z[hi - 1] = omega.argmax()
        for t in range(hi - lo - 1, 0, -1):
            z[lo + t - 1] = phi[t, z[lo + t]]
    return z, tie


def decode(x, q, ln_pi, ln_a, off, order=None, pivot=None):
    from bayesml_amd import _kside
    from bayesml_amd._engine import DataPass
    dev, (K, D) = torch.device("cuda", 0), q.m.shape
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)   # noqa: E731
    f = _kside.features(_kside.PostT(torch.ones(K, dtype=torch.float64, device=dev), t(q.m), t(q.kappa), t(q.nu), t(q.w_inv)))
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    eng = DataPass(K, D, xd.dtype, x.shape[0], dev)
    eng.set_pivot(t(x.mean(axis=0) if pivot is None else pivot))
    eng.prepare_rows(xd)
    eng.set_params((f.e_ln_lambda_det - D * _kside.LN_2PI - D / f.kappa) / 2.0, f.m, f.u)
    eng.enable_hmm()
    assert eng.emission_target(False) is False
    eng.estep(xd)
    ln_rho = eng.ln_rho().cpu().numpy()
    off_dev, order_dev = eng.segment_tables(off)
    order_dev = order_dev if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    z = eng.viterbi_segments(t(ln_pi), t(ln_a), off_dev, order_dev).cpu().numpy()
    assert eng.last_viterbi_pass() == -1
    eng.close()
    return z, ln_rho


def batch(K, S, edge=None):
    lengths = np.array([0 if edge is not None and i == edge % S else LENGTHS[i % 10] for i in range(S)])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return orc.synth_hmm(max(2, K // 2), 2, int(off[-1]), np.float64, seed=K + S, stay=0.8)[0], off


@pytest.mark.parametrize("K, edge", [(1, None), (4, 0), (5, None), (8, None), (9, -1), (16, None), (17, None), (32, None),
                                     (33, None), (48, None), (64, None)])
def test_paths_against_the_per_segment_recursion(K, edge):
    """S = 4 G + 1: a full workgroup and a one-member wave in a second one, at every Kq and on both sides of each step."""
    (x, off), q = batch(K, 4 * (64 // next(k for k in (4, 8, 16, 32, 64) if k >= K)) + 1, edge), random_posterior(K, 2)
    z, ln_rho = decode(x, q, q.ln_pi_tilde, q.ln_a_tilde, off)
    assert np.array_equal(z, viterbi_reference(ln_rho, q.ln_pi_tilde, q.ln_a_tilde, off)[0])


@pytest.mark.parametrize("K", [5, 17])
def test_ties_take_the_first_maximiser(K):
    """Identical components and uniform zeta: every state scores alike, every maximum is a tie."""
    (x, off), q = batch(K, 4 * (64 // (8 if K == 5 else 32)) + 1), random_posterior(K, 2)
    q.m[:], q.w[:], q.w_inv[:], q.nu[:], q.kappa[:] = q.m[0], q.w[0], q.w_inv[0], q.nu[0], q.kappa[0]
    q.eta[:], q.zeta[:] = 2.0, 2.0
    q.refresh()
    z, ln_rho = decode(x, q, q.ln_pi_tilde, q.ln_a_tilde, off)
    ref, tie = viterbi_reference(ln_rho, q.ln_pi_tilde, q.ln_a_tilde, off)
    assert tie and np.array_equal(z, ref)


def test_order_independence():
    """Order reversed, and sequences permuted together with their rows under one pivot: every sequence's path is the same."""
    (x, off), q = batch(17, 9), random_posterior(17, 2)
    S, pivot, pi, a = len(off) - 1, x.mean(axis=0), q.ln_pi_tilde, q.ln_a_tilde
    z = decode(x, q, pi, a, off, pivot=pivot)[0]
    perm = np.random.default_rng(17).permutation(S)
    rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in perm])
    per = decode(x[rows], q, pi, a, np.concatenate([[0], np.cumsum(np.diff(off)[perm])]), pivot=pivot)[0]
    assert np.array_equal(decode(x, q, pi, a, off, order=np.arange(S)[::-1], pivot=pivot)[0], z) and np.array_equal(per, z[rows])


@pytest.mark.parametrize("K, D, T", [(4, 2, 120), (40, 2, 300)])
def test_estimate_latent_vars_over_many_sequences(K, D, T):
    """The model level on the inputs of test_gpu_hmm.py's test_viterbi_kernel_against_oracle."""
    from bayesml_amd import hiddenmarkovnormal as hmm
    x, _ = orc.synth_hmm(max(2, K // 2), D, T, np.float64, seed=7 * K + T)
    m = hmm.LearnModel(K, D, seed=1, verbose=False)
    rng = np.random.default_rng(K)
    m.set_hn_params(hn_eta_vec=rng.uniform(0.5, 5, K), hn_zeta_vecs=rng.uniform(0.5, 5, (K, K)) + 3 * np.eye(K),
                    hn_m_vecs=3.0 * rng.standard_normal((K, D)))
    q = orc.HmmPosterior(m.hn_eta_vec.copy(), m.hn_zeta_vecs.copy(), m.hn_m_vecs.copy(), m.hn_kappas.copy(),
                         m.hn_nus.copy(), m.hn_w_mats.copy(), m.hn_w_mats_inv.copy()).refresh()
    lengths = np.array([7, 0, 1, 30] + [(T - 38) // 2, T - 38 - (T - 38) // 2])
    off = np.concatenate([[0], np.cumsum(lengths)])
    pieces = [(lo, hi) for lo, hi in zip(off[:-1], off[1:]) if hi > lo]
    z = m.estimate_latent_vars(x, "0-1", viterbi=True, lengths=lengths)
    assert np.array_equal(z, np.vstack([orc.viterbi(x[lo:hi], q) for lo, hi in pieces]))
    assert not np.array_equal(z, m.estimate_latent_vars(x, "0-1", viterbi=True))          # the junction error is real
    ln_rho = orc.emission_ln_rho(x, q)
    rho = np.exp(ln_rho - ln_rho.max(axis=1, keepdims=True))
    gamma = np.vstack([np.multiply(*orc.forward_backward(rho[lo:hi], q.pi_tilde, q.a_tilde)[:2]) for lo, hi in pieces])
    assert np.max(np.abs(m.estimate_latent_vars(x, "squared", viterbi=False, lengths=lengths) - gamma)) < 1e-7
