"""The sequential multivariate-normal kernels (csrc/mvnseq_kernels.h) on the GPU at the edges of their branches: every length
of the cut last block in both K paths and nothing written past it, every slice count of the binary64 K path, the restart in
double-double above kDdThreshold (mvn_seq_cases.py) also across pass boundaries, the ends of the code length's ranges and
the switch of its lnGamma step at a large D / 2, a second call on a model, and passes over strided f32 rows at D > 16.

Oracle and bound are those of test_gpu_mvn_seq.py (mvn_seq_oracle.check): the long-double row loop, 8 x the float64 row
loop's own error on the same rows and never below 64 eps, separately for the first 2 D rows and the rest.  Every test prints
worst error / tolerance; the measured figures are in profiles/mvnseq.md, those of the NumPy block form on the same cases in
test_mvn_seq_edges.py.
"""
import numpy as np
import pytest
import torch

import mvn_seq_cases as cases
import mvn_seq_oracle as seq

pytestmark = pytest.mark.gpu

B = seq.BLOCK


# ---- the cut last block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 40))
def test_every_cut(D):
    """Calls on the first n rows of one sample for every n up to 66 (each ramp block as the cut block; no row, one row and
    two rows in the first block of 64) and for 63 + L rows, L around every multiple of 16: the wave boundaries of ``valid``
    and ``rowc``.  The block at row 63 starts past 2 D rows at D = 3 (binary64 K on the matrix pipe) and within them at
    D = 40 (double-double)."""
    x, start = cases.cut_case(D)
    seq.sweep(f"D = {D}", D, cases.cut_ns(), x, start)


def run_pass(lib, D, x, start, n, pm, logdet, quad, nats):
    """One mvnseq_pass over all n rows of the f64 device matrix x into the given outputs (tensors or None)."""
    from bayesml_amd import _mvnseq
    d = seq.dev()
    carry = torch.zeros(D * D + D + 1, dtype=torch.float64, device=d)
    work = torch.empty(_mvnseq.work_slots(D, _mvnseq.block_count(n)), dtype=torch.float64, device=d)
    ptr = [None if o is None else o.data_ptr() for o in (pm, logdet, quad, nats)]
    with torch.cuda.device(d):
        _mvnseq._check(lib.mvnseq_pass(D, 1, x.data_ptr(), D, n, 0, n, start.data_ptr(), carry.data_ptr(), ptr[0], D, ptr[1],
                                       ptr[2], ptr[3], work.data_ptr(), _mvnseq.stream_ptr(d)), "mvnseq_pass")
    torch.cuda.synchronize(d)


@pytest.mark.parametrize("L", cases.CUTS)
def test_rows_past_the_end_write_nothing(L):
    """mvnseq_pass itself on 63 + L rows at D = 3, p_m [n + 64, D] and the three row outputs [n + 64] filled with NaN: the
    tails are still NaN afterwards and the first n rows are the model's, bit for bit.  At L = 17 also with p_m and two of
    the three row outputs null, in turn: the surviving output is the full call's, bit for bit."""
    from bayesml_amd import _mvnseq
    D, n = 3, B - 1 + L
    x, start = cases.cut_case(D)
    m = seq.model(D, start)
    means, nats = m.pred_and_update_sequence(x[:n], code_length=True)
    base = seq.outputs(m, nats)
    lib, d = _mvnseq.load_library(), seq.dev()
    xd = torch.from_numpy(x[:n]).to(d)
    sd = torch.from_numpy(_mvnseq.start_state(start[3], start[0], start[1], start[2])).to(d)
    fresh = lambda: [torch.full((n + B, D) if k == 0 else (n + B,), np.nan, dtype=torch.float64, device=d)      # noqa: E731
                     for k in range(4)]
    outs = fresh()
    run_pass(lib, D, xd, sd, n, *outs)
    full = [o.cpu().numpy() for o in outs]
    assert all(np.all(np.isnan(o[n:])) for o in full)
    assert all(np.array_equal(o[:n], b) for o, b in zip(full, base))
    if L != 17:
        return
    for keep in (1, 2, 3):
        outs = [o if k == keep else None for k, o in enumerate(fresh())]
        run_pass(lib, D, xd, sd, n, *outs)
        assert np.array_equal(outs[keep].cpu().numpy(), full[keep], equal_nan=True)


# ---- the slices of the binary64 K path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,kind", cases.SLICES)
def test_every_slice_count(D, kind):
    """nt = 4, 4, 5, 8, 16 slices of sixteen columns with K accumulated on the matrix pipe, and the block-start factor over
    as many tiles on S_0 plus a Gram prefix of ``first`` rows and more: the sample reaches one whole block and a cut one of
    17 rows past the first block that starts at or after 2 D rows.  At D = 64 and 128 (D a multiple of 16: no padding
    between the factor and the tail of the state area) also from a correlated S_0 with m_0 != 0, kappa_0 = 2.5 and
    nu_0 = D + 1.75.  From D = 128 on the loops factorise at a subset of the rows (mvn_seq_cases.slice_rows)."""
    first = cases.slice_first(D)
    assert first == cases.FIRST[D]
    x, start = cases.slice_case(D, kind)
    assert len(x) == first + B + 17
    seq.sweep(f"D = {D} {kind}", D, (len(x),), x, start, rows=cases.slice_rows(D))


# ---- the restart above kDdThreshold --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_threshold_restart(name):
    """The onset block of late column, late dummy and outlier has K_ii of 1e6 and more past the first 2 D rows: its slices
    run a second time, in double-double (test_mvn_seq_edges.py: without that the two late cases miss the bound by factors of
    1e4 and more); the control's has 12 and stays on the matrix pipe."""
    x, start = cases.make(name)
    seq.sweep(name, cases.D, (cases.N,), x, start)


def in_passes(D, x, start=None):
    """Passes of 1 and of 3 blocks against one pass: both returns, the traces and hn_* bit-equal.  The one-pass model and
    its returns on the host."""
    from bayesml_amd import _mvnseq
    host = lambda out: [torch.as_tensor(a).cpu().numpy() for a in out]      # noqa: E731
    one = seq.model(D, start)
    base = host(one.pred_and_update_sequence(x, code_length=True))
    assert one._seq_engine.passes == 1
    for blocks in (1, 3):
        m = seq.model(D, start)
        got = host(m.pred_and_update_sequence(x, code_length=True, chunk_bytes=seq.budget_for(D, blocks)))
        assert m._seq_engine.passes == -(-_mvnseq.block_count(len(x)) // blocks) > 1
        assert all(np.array_equal(a, b) for a, b in zip(got, base)) and np.array_equal(m.p_m_vecs, one.p_m_vecs)
        assert np.array_equal(m.p_v_logdets, one.p_v_logdets) and np.array_equal(m.p_quads, one.p_quads)
        assert seq.hn_equal(m, one)
    return one, base


def test_threshold_restart_in_passes():
    """The late column in passes of 1 and of 3 blocks.  The decision to restart is a function of the block's rows and start
    state, and the start state is what a pass boundary hands over: the onset block [63, 127), block 6 of the schedule, is a pass of its own and
    the first block of a pass of three, its Gram prefix coming from the carry alone."""
    x, start = cases.make("late column")
    in_passes(cases.D, x, start)


# ---- the code length -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CODE_LENGTH)
def test_code_length_edges(name):
    """nu_0 at which a = p_nu / 2 passes 64 between two rows and is 64 exactly at row 1, nu_0 just above D - 1 and very
    large, kappa_0 and |x| at 1e-6 and 1e6, repeated and zero rows, and all rows equal - there q is tiny where the clamp at 0
    acts, and p_quads must be exactly 0 wherever the oracle's is.  nu_0 = 1e6 is paired with S_0 = I: with S_0 = 1e6 I,
    D ln(kappa p_nu / (kappa + 1)) and ln det S cancel to order one, and the block form itself misses the floored-at-1 bound
    on p_v_logdets by 5 % - a property of the formula, not of a kernel."""
    x, start = cases.code_length_case(name)
    exact_quad = np.asarray(seq.ld_row_loop(x, *start)[3])
    m = seq.model(cases.D, start)
    m.pred_and_update_sequence(x, code_length=True)
    assert not m.p_quads[exact_quad == 0].any()
    seq.sweep(name, cases.D, (cases.N,), x, start)


@pytest.mark.parametrize("D", (128, 256))
def test_code_length_switch_at_large_D(D):
    """nu_0 = D + 120: a = p_nu / 2 reaches 64 at row 7 with h = D / 2 = 64 and 128; one row past the first block of 64.
    The loops factorise at the first 20 rows and around row 63."""
    x, start = cases.switch_case(D)
    seq.sweep(f"switch D = {D}", D, (len(x),), x, start, rows=cases.SWITCH_ROWS)


# ---- a second call on a model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", (1, 5, 100))
def test_second_call(n1):
    """Rows [0, n1) and [n1, n) in two calls from a diffuse start: the second call's pivot is its own first row, m_0 is not
    the pivot, kappa_0 is not 1, and after 1 and after 5 rows S_0 is still singular to working precision."""
    x, start = cases.second_call_case()
    seq.second_call(f"second call after {n1} rows", cases.D, x, start, n1)


# ---- passes ------------------------------------------------------------------------------------------------------------------
def test_passes_on_strided_f32():
    """D = 33 on f32 rows that lie in a [n, D + 3] device matrix, in passes of 1 and of 3 blocks against one pass: the
    pass-relative indices of mean_rel and scale and the slab index of the Gram scan at T > 1 are cut by a pass.  The one
    pass is held to the bound as the widened rows."""
    x, start = cases.strided_case()
    n, D = x.shape
    wide = torch.zeros((n, D + 3), dtype=torch.float32, device=seq.dev())
    wide[:, :D] = torch.from_numpy(x)
    assert wide[:, :D].stride(0) == D + 3
    one, base = in_passes(D, wide[:, :D], start)
    x = x.astype(np.float64)
    worst = seq.check("D = 33 strided f32", (base[0], one.p_v_logdets, one.p_quads, base[1]), seq.pick(seq.ld_row_loop(x, *start)),
                      seq.pick(seq.row_loop(x, *start)), x, D)
    print(f"D = 33 strided f32: worst error / tolerance {worst:.2f}")
