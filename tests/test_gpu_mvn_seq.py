"""``pred_and_update_sequence`` of multivariate_normal on the device (include/mvnseq.h), against the long-double loop at
the bound of tests/mvn_seq_oracle.py: within 8 x the float64 reference loop's own error on the same rows, never below 64 eps,
the first 2 D rows and the rest judged separately; p_quads relative per row, nats and p_v_logdets relative with the magnitude
floored at 1, the means relative to max |x|.  Every test prints worst error / tolerance (profiles/mvnseq.md has them).
"""
import ctypes

import numpy as np
import pytest
import torch

import mvn_seq_oracle as seq
from conftest import load_golden
from mvn_seq_oracle import budget_for, default_start, dev, model, outputs, sweep, synth

pytestmark = pytest.mark.gpu
B = seq.BLOCK


@pytest.mark.parametrize("name", seq.FIXTURES)
def test_fixtures(name):
    g = load_golden(name)
    x, start, exact, ref = seq.fixture_parts(g)
    n, D = x.shape
    m = model(D, start)
    means, nats = m.pred_and_update_sequence(x, code_length=True)
    assert np.array_equal(m.p_nus, g["ref_p_nu"]) and means is m.p_m_vecs
    print("worst error / tolerance: %.2f" % seq.check(name, outputs(m, nats), exact, ref, x, D))
    assert np.allclose(m.hn_w_mat_inv, g["hn_w_mat_inv"], rtol=1e-9, atol=1e-12) and m.hn_nu == float(g["hn_nu"])


@pytest.mark.parametrize("D", (1, 2, 15, 16, 17, 33, 128, 256))
def test_shapes(D):
    """n on both sides of the block edges; from D = 128 on the four shortest only, the long-double loop on a subset of the
    rows: both sides of every block edge and the first 2 D rows."""
    ns = (1, B - 1, B, B + 1) if D >= 128 else (1, B - 1, B, B + 1, 3 * B + 17)
    x = synth(D, ns[-1], 400 + D)
    rows = None
    if D >= 128:
        edges = seq.schedule(ns[-1])
        rows = sorted({i for e in edges for i in (e - 1, e) if 0 <= i < ns[-1]} | set(range(min(2 * D, ns[-1]))))
    sweep(f"D = {D}", D, ns, x, default_start(D), rows=rows)


@pytest.mark.parametrize("case", ("diffuse", "tight", "constant column"))
def test_hard_cases(case):
    """A diffuse start (S_0 = 1e-6 I: what the leading ramp is for), a tight sample far from the origin (mean 1e6, spread
    1e-2: what the pivot is for), and a column that is constant for the first 100 rows (S is rank-deficient apart from
    S_0 until then, and the column switches on inside the block [63, 127))."""
    D, n = 8, 3 * B + 17
    start = default_start(D)
    if case == "diffuse":
        x, start = synth(D, n, 500), (np.zeros(D), 1.0, float(D), np.eye(D) * 1e-6)
    elif case == "tight":
        x = synth(D, n, 501, loc=1e6, spread=1e-2)
    else:
        x = synth(D, n, 502)
        x[:100, 3] = x[0, 3]
    sweep(case, D, (n,), x, start)


def test_passes_are_bit_equal_to_one_call():
    """chunk_bytes for 1 and for 3 blocks per pass against the default, and explicit mvnseq_pass calls on the cuts
    [0, 2, 3, 7, end]; the carry is [G | sum (x - pivot) | n] of all rows."""
    from bayesml_amd import _mvnseq
    D, n = 5, 3 * B + 17
    x = synth(D, n, 600)
    one = model(D)
    base = one.pred_and_update_sequence(x, code_length=True)
    assert one._seq_engine.passes == 1
    for blocks in (1, 3):
        m = model(D)
        got = m.pred_and_update_sequence(x, code_length=True, chunk_bytes=budget_for(D, blocks))
        assert m._seq_engine.passes == -(-_mvnseq.block_count(n) // blocks) > 1
        assert all(np.array_equal(a, b) for a, b in zip(got, base))
        assert np.array_equal(m.p_v_logdets, one.p_v_logdets) and np.array_equal(m.p_quads, one.p_quads)
        assert seq.hn_equal(m, one)
    lib, d = _mvnseq.load_library(), dev()
    xd = torch.from_numpy(x).to(d)
    start = torch.from_numpy(_mvnseq.start_state(np.eye(D), np.zeros(D), 1.0, float(D))).to(d)
    carry = torch.zeros(D * D + D + 1, dtype=torch.float64, device=d)
    pm = torch.full((n, D), np.nan, dtype=torch.float64, device=d)
    logdet, quad, nats = (torch.full((n,), np.nan, dtype=torch.float64, device=d) for _ in range(3))
    cuts = [0, 2, 3, 7, _mvnseq.block_count(n)]                  # passes of 2, 1, 4 blocks and the rest
    work = torch.empty(_mvnseq.work_slots(D, max(np.diff(cuts))), dtype=torch.float64, device=d)
    with torch.cuda.device(d):
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            r0, r1 = _mvnseq.block_start(n, b0), _mvnseq.block_start(n, b1)
            _mvnseq._check(lib.mvnseq_pass(D, 1, xd.data_ptr(), D, n, r0, r1 - r0, start.data_ptr(), carry.data_ptr(),
                                           pm.data_ptr(), D, logdet.data_ptr(), quad.data_ptr(), nats.data_ptr(),
                                           work.data_ptr(), _mvnseq.stream_ptr(d)), "mvnseq_pass")
    assert np.array_equal(pm.cpu().numpy(), base[0]) and np.array_equal(nats.cpu().numpy(), base[1])
    assert np.array_equal(logdet.cpu().numpy(), one.p_v_logdets) and np.array_equal(quad.cpu().numpy(), one.p_quads)
    want = seq.ld_carry(x, *default_start(D)).astype(np.float64)
    got = carry.cpu().numpy()
    print("carry: worst difference %.1e" % np.max(np.abs(got - want)))
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13) and got[-1] == n
    assert np.array_equal(one._seq_engine.carry.cpu().numpy(), got)


def test_dtypes_and_strides():
    """f32 and f64, a NumPy array, a device tensor and a row-strided view: device tensors are read where they lie, and
    every output is that of the widened contiguous copy, bit for bit."""
    D, n = 7, 2 * B + 5
    x = synth(D, n, 700)
    for xt in (np.float32, np.float64):
        xs = x.astype(xt)
        b = model(D)
        base = b.pred_and_update_sequence(xs.astype(np.float64), code_length=True)
        wide = torch.zeros((n, D + 3), dtype=torch.from_numpy(xs).dtype, device=dev())
        wide[:, :D] = torch.from_numpy(xs)
        for xa in (xs, torch.from_numpy(xs).to(dev()), wide[:, :D]):
            m = model(D)
            got = m.pred_and_update_sequence(xa, code_length=True)
            assert all(isinstance(a, type(xa) if isinstance(xa, np.ndarray) else torch.Tensor) for a in got)
            assert all(np.array_equal(torch.as_tensor(a).cpu().numpy(), c) for a, c in zip(got, base))
            assert np.array_equal(m.p_v_logdets, b.p_v_logdets) and np.array_equal(m.p_quads, b.p_quads)
            if not isinstance(xa, np.ndarray):
                assert got[0].device == dev() and got[0].dtype == torch.float64


def test_two_runs_are_bit_equal():
    D, n = 40, 5 * B + 3
    x = synth(D, n, 800)
    a, b = model(D), model(D)
    ra = a.pred_and_update_sequence(x, code_length=True)
    rb = b.pred_and_update_sequence(x, code_length=True)
    assert all(np.array_equal(u, v) for u, v in zip(ra, rb)) and seq.hn_equal(a, b)
    assert np.array_equal(a.p_v_logdets, b.p_v_logdets) and np.array_equal(a.p_quads, b.p_quads)


def test_null_outputs():
    """loss=None asks for no means: p_m_vecs is None and the code lengths are the full call's bits."""
    D, n = 9, 2 * B + 1
    x = synth(D, n, 850)
    full = model(D)
    _means, nats = full.pred_and_update_sequence(x, code_length=True)
    m = model(D)
    alone = m.pred_and_update_sequence(x, loss=None, code_length=True)
    assert m.p_m_vecs is None and np.array_equal(alone, nats)
    assert np.array_equal(m.p_v_logdets, full.p_v_logdets) and np.array_equal(m.p_quads, full.p_quads)
    assert seq.hn_equal(m, full)


def test_invalid_arguments():
    from bayesml_amd import _mvnseq
    lib, d = _mvnseq.load_library(), dev()
    D, n = 4, 200
    buf = torch.zeros(max(_mvnseq.work_slots(D, _mvnseq.block_count(n)), n * D), dtype=torch.float64, device=d)
    P = ctypes.c_void_p(buf.data_ptr())

    def call(D=D, ldx=D, begin=0, count=n, work=P):
        return lib.mvnseq_pass(D, 1, P, ldx, n, begin, count, P, P, None, D, None, None, P, work, None)

    for kw in (dict(D=0), dict(D=257, ldx=257), dict(begin=2, count=198), dict(begin=0, count=100), dict(ldx=3),
               dict(work=None)):
        assert call(**kw) == 1, (kw, lib.mvnseq_last_error())
    torch.cuda.synchronize()
    assert not buf.any()                      # nothing was launched


def test_a_long_sample_in_several_passes():
    """n = 200 003 at D = 16, f32, with loss=None under an 8 MiB budget: finite code lengths whose sum is -ln p(X) of the
    end state, within 64 eps x the magnitudes summed on both sides."""
    D, n = 16, 200003
    x = synth(D, n, 900).astype(np.float32)
    m = model(D)
    nats = m.pred_and_update_sequence(x, loss=None, code_length=True, chunk_bytes=8 << 20)
    assert m._seq_engine.passes > 1 and nats.shape == (n,) and np.all(np.isfinite(nats)) and m.p_m_vecs is None
    assert np.all(np.isfinite(m.p_v_logdets)) and np.all(m.p_quads >= 0) and m.hn_kappa == 1.0 + n
    lml, terms = seq.log_marginal(D, n, 1.0, float(D), np.eye(D), m.hn_kappa, m.hn_nu, m.hn_w_mat_inv)
    bound = 64 * seq.EPS * (np.abs(nats).sum() + np.abs(terms).sum())
    print(f"sum nats + ln p(X) = {nats.sum() + lml:.2e}, bound {bound:.2e}, passes {m._seq_engine.passes}")
    assert abs(nats.sum() + lml) <= bound
