"""The cases of test_gpu_mvn_seq_edges.py on the CPU: the NumPy block form (mvn_seq_oracle.block_form, directly and behind the
model's stand-in) against the long-double loop at the bound of mvn_seq_oracle.check, so that the bound is known to be fair
before a GPU sees it; the branch each case is meant to take, from ``block_form(..., diag=...)``; that the double-double
threshold is what holds the late-onset cases to the bound; and the code length's lnGamma step on both sides of its switch.

Measured on a CPU, worst error / tolerance of the block form: every cut 0.24 (D = 3) and 0.16 (D = 40); slice counts 0.10
to 0.30 (D = 128 default); late column 0.25, late dummy 0.61, control 0.15, outlier 0.23; code-length edges 0.04 to 0.23
(x 1e6); the switch at D = 128 and 256 0.12 and 0.16; second call after 1, 5, 100 rows 0.19, 0.13, 0.36; D = 33 f32 0.40.
"""
import numpy as np
import pytest

import mvn_seq_cases as cases
import mvn_seq_oracle as seq

B = seq.BLOCK


def held(label, x, start, rows=None, **kw):
    """block_form on (x, start) against both loops at the bound: (outputs, exact, ref, diag)."""
    exact = seq.pick(seq.ld_row_loop(x, *start, rows=rows))
    ref = seq.pick(seq.row_loop(x, *start, rows=rows))
    diag = []
    got = seq.pick(seq.block_form(x, seq.state_of(start), diag=diag, **kw))
    print(f"{label}: worst error / tolerance {seq.check(label, got, exact, ref, x, x.shape[1], rows=rows):.2f}")
    return got, exact, ref, diag


# ---- the threshold restart -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_threshold_cases(name):
    """The onset block of late column, late dummy and outlier starts past the first 2 D rows with max K_ii above the
    threshold (measured: 1.07e7, 9.9e5, 2.0e7), and no other block past them does; every block of the control stays below
    it (12 at most).  With the data out of the decision the two late cases miss the bound (p_quad errors 2.6e-8 and 3.2e-9
    against 6e-13 and 1.4e-14).  The outlier passes either way - its S_c is well conditioned, one row is far out - and is
    here for the restart's code, not for its precision: nothing is asserted about it without the threshold."""
    x, start = cases.make(name)
    got, exact, ref, diag = held(name, x, start)
    flagged = [(lo, hi) for lo, hi, head, k in diag if not head and k > seq.DD_THRESHOLD]
    print(f"{name}: K_ii past the first 2 D rows " + ", ".join(f"[{lo}, {hi}) {k:.3g}" for lo, hi, head, k in diag if not head))
    if name == "control":
        assert flagged == []
        return
    blk = cases.onset_block(name)
    assert blk.start >= 2 * cases.D and flagged == [(blk.start, blk.stop)]
    assert (blk.start, blk.stop) == ((127, 191) if name == "outlier" else (63, 127))
    if name == "late column":
        assert not x[:100, 3].any() and not got[0][:101, 3].any()        # u_3 is exactly 0 before row 100
    if name != "outlier":
        old = seq.pick(seq.block_form(x, seq.state_of(start), dd_threshold=None))
        with pytest.raises(AssertionError):
            seq.check(name + " (rows alone decide)", old, exact, ref, x, cases.D)


def test_threshold_restart_in_passes():
    x, start = cases.make("late column")
    one = seq.block_form(x, seq.state_of(start))
    for per in (1, 3):
        assert all(np.array_equal(a, b) for a, b in zip(one, seq.block_form(x, seq.state_of(start), blocks_per_pass=per)))


# ---- the cut last block ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 40))
def test_every_cut(D):
    """Through the model on the stand-in, as the GPU test goes through the model on the device.  The block at row 63 is past
    the first 2 D rows at D = 3 and within them at D = 40."""
    x, start = cases.cut_case(D)
    assert (B - 1 >= 2 * D) == (D == 3) and max(cases.cut_ns()) <= len(x)
    seq.sweep(f"D = {D}", D, cases.cut_ns(), x, start, make_model=seq.model_at)


# ---- the slices of the binary64 K path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,kind", cases.SLICES)
def test_every_slice_count(D, kind):
    """The block at ``first`` and the cut one after it are past the first 2 D rows with K_ii far below the threshold
    (measured: 2.1 at most): binary64 K on the matrix pipe, over nt = 4, 4, 5, 8, 16 slices."""
    first = cases.slice_first(D)
    assert first == cases.FIRST[D]
    x, start = cases.slice_case(D, kind)
    rows = cases.slice_rows(D)
    if rows is not None:
        n, edges = len(x), [b for b in seq.schedule(len(x)) if b >= first]
        assert set(range(16)) | set(range(2 * D - 4, 2 * D + 5)) | {n - 1} <= set(rows)
        assert all(i in rows for e in edges for i in (e - 1, e) if i < n)
        assert all(any(i + k in rows for k in range(4) if i + k < n) for i in range(first, n))
    diag = held(f"D = {D} {kind}", x, start, rows=rows)[3]
    tail = [(lo, hi, head, k) for lo, hi, head, k in diag if lo >= first]
    assert [(lo, hi) for lo, hi, _h, _k in tail] == [(first, first + B), (first + B, first + B + 17)]
    assert all(not head and k < seq.DD_THRESHOLD for _lo, _hi, head, k in tail)


# ---- the code length ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CODE_LENGTH)
def test_code_length_edges(name):
    x, start = cases.code_length_case(name)
    got, exact, _ref, _diag = held(name, x, start)
    zero = np.asarray(exact[2]) == 0
    assert not got[2][zero].any()


@pytest.mark.parametrize("D", (128, 256))
def test_code_length_switch_at_large_D(D):
    x, start = cases.switch_case(D)
    p_nu = start[2] + np.arange(len(x)) - D + 1
    assert p_nu[6] / 2 < 64.0 == p_nu[7] / 2
    held(f"switch D = {D}", x, start, rows=cases.SWITCH_ROWS)


@pytest.mark.parametrize("h", (0.5, 8.0, 64.0, 128.0))
def test_lgamma_step(h):
    """lnGamma(a) - lnGamma(a + h) as the kernel evaluates it, against the long-double series, on both sides of the switch
    at a = 64 and far above it.  Bound: 64 eps of the value, its magnitude floored at 1 - the floor of the bound the rows'
    code lengths are held to; from a = 64 on the Stirling difference has no term much larger than its value (at most
    h ln(a + h) + h against a value of at least h ln(a + h) - h / 2), so a few roundings of the terms stay far inside it.
    Below 64 the value is the difference of two rounded lgamma values, as in the reference, and the bound is never below
    two ulps of each of them and of their difference.  The oracle is itself a difference of two long-double values of up to
    6e6 (a = 5e5), each rounded: two long-double ulps of them are added to the bound (5e-13 there, 1e-17 at a = 64)."""
    a = np.array([63.5, 64 - 2.0 ** -40, 64.0, 64.5, 1e3, 5e5])
    exact = seq.ld_lgamma(a) - seq.ld_lgamma(a.astype(seq.LD) + seq.LD(h))
    got = seq.lgamma_step(a, h)
    mag = np.abs(exact).astype(np.float64)
    tol = 64 * seq.EPS * np.maximum(mag, 1.0)
    parts = np.abs(seq.ld_lgamma(a)) + np.abs(seq.ld_lgamma(a + h)) + np.abs(exact)
    tol = np.where(a < 64.0, np.maximum(tol, 2 * seq.EPS * parts.astype(np.float64)), tol)
    tol = tol + 2 * float(np.finfo(seq.LD).eps) * parts.astype(np.float64)          # the oracle's own two roundings
    err = np.abs(got.astype(seq.LD) - exact).astype(np.float64)
    print(f"h = {h}: " + ", ".join(f"a = {v:.12g} {e:.1e} / {t:.1e}" for v, e, t in zip(a, err, tol)))
    assert np.all(err <= tol)
    assert a[1] < 64.0 and abs(got[1] - got[2]) <= tol[1] + tol[2] + 2.0 ** -40 * np.log1p(h / 64.0) * 1.1


# ---- a second call, passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", (1, 5, 100))
def test_second_call(n1):
    x, start = cases.second_call_case()
    seq.second_call(f"second call after {n1} rows", cases.D, x, start, n1, make_model=seq.model_at)


def test_passes_on_f32_rows():
    """The D = 33 sample of the strided GPU test: held to the bound as the widened rows, and bit-equal in passes."""
    x, start = cases.strided_case()
    x = x.astype(np.float64)
    held("D = 33 f32", x, start)
    one = seq.block_form(x, seq.state_of(start))
    for per in (1, 3):
        assert all(np.array_equal(a, b) for a, b in zip(one, seq.block_form(x, seq.state_of(start), blocks_per_pass=per)))
