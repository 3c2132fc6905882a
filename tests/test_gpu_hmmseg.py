"""The HMM forward-backward pass over many sequences laid end to end (csrc/hmmseg_kernels.h) against the oracle's own parts
applied to every segment on its own.  Tolerances of tests/test_gpu_hmm.py: 1e-10 on alpha, gamma, g0, gl; 1e-9 relative on sums."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import hmm_vb_oracle as orc

pytestmark = pytest.mark.gpu


def random_posterior(K, D):
    """The random posterior of test_ragged_shapes_against_oracle."""
    rng = np.random.default_rng(100 * K + D)
    q = orc.HmmPosterior.from_prior(orc.HmmPrior.default(K, D))
    q.m = 3.0 * rng.standard_normal((K, D))
    a = rng.standard_normal((K, D, D))
    q.w_inv = a @ np.swapaxes(a, 1, 2) + D * np.eye(D)
    q.w = np.linalg.inv(q.w_inv)
    q.nu, q.kappa = q.nu + rng.uniform(0, 3, K), q.kappa + rng.uniform(0, 3, K)
    q.eta, q.zeta = q.eta + rng.uniform(0, 5, K), q.zeta + rng.uniform(0, 5, (K, K)) + 4 * np.eye(K)
    return q.refresh()


def segment_oracle(x, q, off):
    """forward_backward on exp(ln rho - row max) of every segment on its own; xi summed over t > first; g0 / gl summed."""
    T, K = x.shape[0], q.m.shape[0]
    ln_rho = orc.emission_ln_rho(x.astype(np.float64), q)
    mx = ln_rho.max(axis=1, keepdims=True)
    rho = np.exp(ln_rho - mx)
    alpha, gamma, cs = np.zeros((T, K)), np.zeros((T, K)), np.ones(T)
    ms, g0, gl = np.zeros((K, K)), np.zeros(K), np.zeros(K)
    for lo, hi in zip(off[:-1], off[1:]):
        if hi > lo:
            a, b, c = orc.forward_backward(rho[lo:hi], q.pi_tilde, q.a_tilde)
            alpha[lo:hi], gamma[lo:hi], cs[lo:hi] = a, a * b, c
            ms += (a[:-1].T @ (rho[lo + 1:hi] * b[1:] / c[1:, None])) * q.a_tilde
            g0, gl = g0 + gamma[lo], gl + gamma[hi - 1]
    return dict(ln_rho=ln_rho, alpha=alpha, gamma=gamma, cs=cs * np.exp(mx[:, 0]), ms=ms, g0=g0, gl=gl, ns=gamma.sum(axis=0),
                lnc=float((np.log(cs) + mx[:, 0]).sum()))


def segment_pass(x, q, off, order=None, fused=False, pivot=None, eng=None, keep=False):
    """One data pass over the segments through the C ABI, as device_pass of tests/test_gpu_hmm.py runs the single sequence.
    ``eng``: an engine an earlier call left open with ``keep`` (built for at least as many rows); the result then carries it as
    ``eng``.  ``ln_rho`` is the array the engine holds after ``estep`` (None with the fused emission, which forms none)."""
    from bayesml_amd import _kside
    from bayesml_amd._engine import DataPass
    dev, (K, D) = torch.device("cuda", 0), q.m.shape
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)   # noqa: E731
    f = _kside.features(_kside.PostT(torch.ones(K, dtype=torch.float64, device=dev), t(q.m), t(q.kappa), t(q.nu), t(q.w_inv)))
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if eng is None:
        eng = DataPass(K, D, xd.dtype, x.shape[0], dev)
    eng.set_pivot(xd[:4096].to(torch.float64).mean(dim=0) if pivot is None else t(pivot))
    eng.prepare_rows(xd)
    eng.set_params((f.e_ln_lambda_det - D * _kside.LN_2PI - D / f.kappa) / 2.0, f.m, f.u)
    eng.enable_hmm()
    assert eng.emission_target(fused) == fused
    eng.estep(xd)
    ln_rho = None if fused else eng.ln_rho().cpu().numpy()
    off_dev, order_dev = eng.segment_tables(off)
    if order is not None:
        order_dev = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    ms, g0, gl, lnc = eng.forward_backward_segments(t(q.pi_tilde), t(q.a_tilde), off_dev, order_dev)
    out = dict(ms=ms.cpu().numpy(), g0=g0.cpu().numpy(), gl=gl.cpu().numpy(), lnc=float(lnc),
               ns=eng.split_stats(eng.mstep(xd))[0].cpu().numpy(), gamma=eng.responsibilities().cpu().numpy(), alpha=eng.hmm_debug(0).cpu().numpy(),
               cprime=eng.hmm_debug(1).cpu().numpy(), xi=eng.hmm_readout("xi", 0, None, t(q.a_tilde)).cpu().numpy(),
               gate=eng.last_boundary_pass(), ln_rho=ln_rho, eng=eng if keep else None)
    if not keep:
        eng.close()
    return out


def batch(K, D, S, edge=None, dtype=np.float64):
    """S sequences whose lengths cycle through 37, 0, 1, 2, 3, 4, 5, 9 (S = 1: 37 rows), the first or last one empty on request."""
    lengths = np.array([[37, 0, 1, 2, 3, 4, 5, 9][(3 * i) % 8] for i in range(S)])
    if edge is not None:
        lengths[edge] = 0
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return orc.synth_hmm(max(2, K // 2), D, int(off[-1]), dtype, seed=K + S, stay=0.8)[0], off


# K: one to four 16-state blocks, padded; fused (D = 2, 16, K <= 32): rho' from the emission kernel, else hmm_prep_kernel; S: a
# partial / full / second wave, a second workgroup; edge: an empty first / last sequence.  Developer switches: room for four xi
# slabs only (a wave takes a second group of 16, as past 65 600 sequences), and the w_tm path at K <= 32.
CASES = [(3, 2, 17, 0, np.float64, True, None), (16, 16, 16, None, np.float64, True, None),
         (17, 17, 15, None, np.float32, False, None), (33, 2, 65, -1, np.float64, False, None),
         (64, 3, 1, None, np.float64, False, None), (64, 2, 17, 0, np.float64, False, None),
         (17, 2, 65, 0, np.float64, False, "GMMVB_HMMSEG_WAVES"), (17, 2, 65, 0, np.float64, False, "GMMVB_HMM_XI_SEPARATE")]


@pytest.mark.parametrize("K, D, S, edge, dtype, fused, switch", CASES)
def test_data_pass_against_the_per_segment_oracle(K, D, S, edge, dtype, fused, switch, monkeypatch):
    for name in ("GMMVB_DEBUG", switch) if switch else ():
        monkeypatch.setenv(name, "4")
    (x, off), q = batch(K, D, S, edge, dtype), random_posterior(K, D)
    r, o = segment_pass(x, q, off, fused=fused), segment_oracle(x, q, off)
    assert np.max(np.abs(r["alpha"] - o["alpha"])) < 1e-10 and np.max(np.abs(r["gamma"] - o["gamma"])) < 1e-10
    assert np.max(np.abs(r["g0"] - o["g0"])) < 1e-10 and np.max(np.abs(r["gl"] - o["gl"])) < 1e-10
    assert abs(r["lnc"] - o["lnc"]) < 1e-9 * max(1.0, abs(o["lnc"]))
    assert rel_err(r["ms"], o["ms"]) < 1e-9 and rel_err(r["ns"], o["ns"]) < 1e-9
    first = np.unique(off[:-1][np.diff(off) > 0])
    assert abs(r["ms"].sum() - (x.shape[0] - len(first))) < 1e-7 and np.all(r["xi"][first] == 0.0) and r["gate"] == -1


@pytest.mark.parametrize("K", [16, 33])
def test_order_independence(K):
    """Order reversed, and sequences permuted with their rows: each row's alpha, c', gamma bit-equal; ms, g0, gl to the tolerances."""
    (x, off), q = batch(K, 2, 65), random_posterior(K, 2)
    S, pivot = len(off) - 1, x.mean(axis=0)                                 # (one pivot: the emission's bits depend on it)
    o = segment_oracle(x, q, off)
    r = segment_pass(x, q, off, pivot=pivot)
    rev = segment_pass(x, q, off, order=np.arange(S)[::-1], pivot=pivot)
    perm = np.random.default_rng(K).permutation(S)
    rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in perm])
    per = segment_pass(x[rows], q, np.concatenate([[0], np.cumsum(np.diff(off)[perm])]), pivot=pivot)
    for key in ("alpha", "cprime", "gamma"):
        assert np.array_equal(rev[key], r[key]) and np.array_equal(per[key], r[key][rows]), key
    for v in (rev, per):
        assert rel_err(v["ms"], o["ms"]) < 1e-9 and max(np.abs(v["g0"] - o["g0"]).max(), np.abs(v["gl"] - o["gl"]).max()) < 1e-10


def test_the_junction_error_is_visible():
    """17 sequences of 5 rows: the segmented ms is the per-segment oracle's, which is NOT the ms of the same rows as one sequence."""
    off = 5 * np.arange(18, dtype=np.int64)
    x, q = orc.synth_hmm(4, 2, 85, np.float64, seed=5, stay=0.8)[0], random_posterior(4, 2)
    o = segment_oracle(x, q, off)
    assert np.max(np.abs(o["ms"] - segment_oracle(x, q, np.array([0, 85]))["ms"])) > 1e-3
    assert rel_err(segment_pass(x, q, off)["ms"], o["ms"]) < 1e-9


def oracle_fit(x, off, K, D, seed, init_type, max_itr):
    """One restart of the oracle's driver over segments; a leading row (gamma = g0, ln rho = 0) is what lower_bound reads as row 0."""
    from bayesml_amd.hiddenmarkovnormal import LearnModel
    p, rng, T = orc.HmmPrior.default(K, D), np.random.default_rng(seed), x.shape[0]
    q = orc.HmmPosterior.from_prior(p)
    if init_type == "subsampling":
        orc.init_subsampling(x, q, rng)
        o = segment_oracle(x, q, off)
    else:
        gamma, ms, g0, _ = LearnModel._random_segments(rng.dirichlet(np.ones(K * K), T).reshape(T, K, K), off)
        o = dict(gamma=gamma, ms=ms, g0=g0, ln_rho=np.zeros((T, K)), cs=np.ones(T))
    trace, s = [], None
    for it in range(max_itr + 1):
        if it > 0:
            orc.update_q(p, q, st)
            o = segment_oracle(x, q, off)
        ns, ms, x_bar, s = orc.m_step_stats(x, o["gamma"], o["ms"], s)
        st = orc.HmmStats(np.vstack([np.zeros(K), o["ln_rho"]]), None, None, o["cs"], np.vstack([o["g0"], o["gamma"]]), ns, ms,
                          x_bar, s)
        trace.append(orc.lower_bound(p, q, st)["vl"])
    return q, trace


@pytest.mark.parametrize("init_type", ["subsampling", "random_responsibility"])
def test_fit_from_many_sequences(init_type):
    from bayesml_amd import hiddenmarkovnormal as hmm
    K, D, T = 4, 2, 500
    x = load_golden("hmm_c1_sample.npz")["x"][:T]

    def fit(**more):                                             # -> the model and the VL trace it printed
        m, buf = hmm.LearnModel(K, D, seed=7), io.StringIO()
        with redirect_stdout(buf), pytest.warns(Warning):
            m.update_posterior(x, max_itr=3, num_init=1, init_type=init_type, **more)
        return m, [float(s.split("VL: ")[1].split(" ")[0].rstrip("*")) for s in buf.getvalue().split("\r") if "VL: " in s]

    one, plain = fit(lengths=[T])[0], fit()[0]                   # one non-empty sequence is today's call, bit for bit
    assert all(np.array_equal(one.get_hn_params()[k], v) for k, v in plain.get_hn_params().items()) and one.vl == plain.vl
    lengths = np.array([25, 25, 25, 0, 50] + [25] * 15)          # S = 20 against the loop built from the oracle's parts
    off = np.concatenate([[0], np.cumsum(lengths)])
    m, vls = fit(lengths=lengths)
    q, trace = oracle_fit(x.astype(np.float64), off, K, D, 7, init_type, 3)
    assert len(vls) == len(trace) and np.allclose(vls, trace, rtol=1e-8)
    ref = dict(hn_eta_vec=q.eta, hn_zeta_vecs=q.zeta, hn_m_vecs=q.m, hn_kappas=q.kappa, hn_nus=q.nu, hn_w_mats=q.w)
    assert all(rel_err(m.get_hn_params()[key], v) < 1e-8 for key, v in ref.items())
    assert np.all(m.xi_mats[off[:-1][lengths > 0]] == 0.0) and rel_err(m.xi_mats.sum(axis=0), m.ms) < 1e-9
    assert abs(m._gamma_first.sum() - 19) < 1e-9 and abs(m._gamma_last.sum() - 19) < 1e-9
