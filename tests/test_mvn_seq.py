"""``pred_and_update_sequence`` of multivariate_normal on the CPU: the NumPy restatement of the block form
(tests/mvn_seq_oracle.py) against reference-generated fixtures, the schedule and the workspace plan, the C ABI of
include/mvnseq.h without a GPU, and the model's host logic through the ``_mvnseq_pass_factory`` seam.

Tolerance (mvn_seq_oracle.check): an output is compared with the long-double loop and must lie within 8 x the reference
loop's own error on the same rows - from the fixture's ``ref_vs_exact``, separately for the first 2 D rows and for the rest -
and never below 64 eps; relative per row for p_quads, relative with the magnitude floored at 1 for nats and p_v_logdets,
relative to max |x| for the means.  Measured here (worst error / tolerance, the restatement and the model on the stand-in
alike): 0.30 on mvn_seq_d17_posterior (p_v_logdet, first 2 D rows: 1.8e-14 / 6.0e-14), 0.24 and below on the other eight.
"""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import mvn_seq_oracle as seq
from conftest import ROOT, load_golden

B = seq.BLOCK


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", seq.FIXTURES)
def test_block_form_against_the_reference_fixtures(name):
    g = load_golden(name)
    x, start, exact, ref = seq.fixture_parts(g)
    out = seq.block_form(x, seq.state_of(start))
    assert np.array_equal(out[1], g["ref_p_nu"])
    print("worst error / tolerance: %.2f" % seq.check(name, seq.pick(out), exact, ref, x, x.shape[1]))


@pytest.mark.parametrize("name", seq.FIXTURES)
def test_log_marginal_is_the_sum_of_the_reference_code_lengths(name):
    """The formula the long GPU sample is held to, first against a fixture's reference trace.  The diffuse fixtures' first
    2 D reference code lengths are themselves 1e-9 off (``ref_vs_exact``): their sum is held to that."""
    g = load_golden(name)
    x, start, _exact, ref = seq.fixture_parts(g)
    n, D = x.shape
    lml, terms = seq.log_marginal(D, n, start[1], start[2], start[3], float(g["hn_kappa"]), float(g["hn_nu"]), g["hn_w_mat_inv"])
    total = g["ref_nats"].sum()
    bound = 64 * seq.EPS * (np.abs(g["ref_nats"]).sum() + np.abs(terms).sum())
    if "diffuse" in name:
        bound = max(bound, 8 * ref["head"]["nats"] * np.abs(g["ref_nats"][:2 * D]).sum())
    print(f"sum nats + ln p(X) = {total + lml:.2e}, bound {bound:.2e}")
    assert abs(total + lml) <= bound


@pytest.mark.parametrize("per_pass", (1, 2, 7))
def test_block_form_in_passes_is_bit_equal_to_one_pass(per_pass):
    rng = np.random.default_rng(per_pass)
    x = 3.0 + rng.standard_normal((3 * B + 17, 5))
    start = seq.start_state(np.eye(5), np.zeros(5), 1.0, 5.0)
    c1, c2 = [], []
    for a, b in zip(seq.block_form(x, start, carry_out=c1), seq.block_form(x, start, blocks_per_pass=per_pass, carry_out=c2)):
        assert np.array_equal(a, b)
    assert np.array_equal(c1[0], c2[0]) and c1[0][-1] == len(x)


# ---- the schedule, the plan, the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, B - 1, B, B + 1, 3 * B + 17))
def test_schedule(n):
    from bayesml_amd import _mvnseq
    lib = _mvnseq.load_library()
    bounds = seq.schedule(n)
    lengths = np.diff(bounds)
    want = [1 << k for k in range(B.bit_length() - 1)] + [B] * (n // B + 1)
    assert bounds[0] == 0 and bounds[-1] == n and lengths.sum() == n and lengths.min() >= 1
    assert list(lengths[:-1]) == want[:len(lengths) - 1] and lengths[-1] <= want[len(lengths) - 1]
    count = len(bounds) - 1
    assert _mvnseq.block_count(n) == count == lib.mvnseq_block_count(n)
    assert [_mvnseq.block_start(n, b) for b in range(count + 1)] == bounds
    assert [lib.mvnseq_block_start(n, b) for b in range(count + 1)] == bounds
    assert lib.mvnseq_block_start(n, count + 1) == -1 and lib.mvnseq_block_start(n, -1) == -1


def test_plan_and_work_len_agree():
    from bayesml_amd import _mvnseq
    lib = _mvnseq.load_library()
    assert _mvnseq.BLOCK == B
    for D in (1, 16, 17, 33, 128, 255, 256):
        assert lib.mvnseq_block(D) == B
        for blocks in (1, 2, 1000):
            assert _mvnseq.work_slots(D, blocks) == lib.mvnseq_work_len(D, blocks) == seq.work_slots(D, blocks)
        for budget in (1 << 20, 8 << 20, None):
            nb = _mvnseq.plan_blocks(10 ** 6, D, budget)
            limit = _mvnseq.DEFAULT_CHUNK_BYTES if budget is None else budget
            assert nb >= 1 and (nb == 1 or 8 * _mvnseq.work_slots(D, nb) <= limit)
            assert nb == _mvnseq.block_count(10 ** 6) or 8 * _mvnseq.work_slots(D, nb + 1) > limit
        assert _mvnseq.plan_blocks(5, D) == _mvnseq.block_count(5) == 3
    assert lib.mvnseq_block(0) == -1 and lib.mvnseq_block(257) == -1 and lib.mvnseq_block_count(0) == -1
    assert lib.mvnseq_work_len(0, 1) == -1 and lib.mvnseq_work_len(257, 1) == -1 and lib.mvnseq_work_len(4, 0) == -1


def test_header_library_and_ctypes_table_agree():
    from bayesml_amd import _mvnseq
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/mvnseq.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mvnseq_[a-z0-9_]+)\s*\(", text)))
    lib = _mvnseq.load_library()
    assert sorted(_mvnseq.SYMBOLS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.mvnseq_abi_version() == 1 == int(re.search(r"#define MVNSEQ_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"#define MVNSEQ_BLOCK (\d+)", text).group(1)) == B
    assert int(re.search(r"#define MVNSEQ_MAX_DEGREE (\d+)", text).group(1)) == _mvnseq.MAX_DEGREE
    assert "mvnseq_" not in open(ROOT + "/include/regseq.h").read()


def test_argument_errors_without_a_gpu():
    from bayesml_amd import _mvnseq
    lib = _mvnseq.load_library()
    P, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)          # never dereferenced

    def call(D=4, xt=0, x=P, ldx=4, n=200, begin=0, count=200, start=P, carry=P, pm=P, ldpm=4, logdet=None, quad=None,
             nats=None, work=P):
        return lib.mvnseq_pass(D, xt, x, ldx, n, begin, count, start, carry, pm, ldpm, logdet, quad, nats, work, None)

    def refused(rc, text):
        assert rc == 1 and text in lib.mvnseq_last_error().decode(), (rc, lib.mvnseq_last_error())

    refused(call(D=0), "D must be in 1..256")
    refused(call(D=257, ldx=257, ldpm=257), "D must be in 1..256")
    refused(call(xt=2), "x_dtype")
    refused(call(n=0), "n_rows")
    refused(call(ldx=3), "ldx")
    refused(call(ldpm=3), "ld_pm")
    assert call(ldpm=3, pm=None, nats=P, work=None) == 1 and b"null pointer" in lib.mvnseq_last_error()
    for null in ("x", "start", "carry", "work"):
        refused(call(**{null: None}), "null pointer")
    refused(call(xt=1, x=odd), "aligned")
    for name in ("start", "carry", "work", "pm", "logdet", "quad", "nats"):
        refused(call(**{name: odd}), "8-byte aligned")
    # a range that is not whole blocks of the schedule of 200 rows (blocks start at 0, 1, 3, ..., 63, 127, 191)
    refused(call(begin=2, count=198), "not whole blocks")
    refused(call(begin=0, count=100), "not whole blocks")
    refused(call(begin=64, count=63), "not whole blocks")
    refused(call(begin=63, count=138), "not whole blocks")
    refused(call(begin=127, count=0), "row_count")
    refused(call(begin=-1, count=2), "not whole blocks")


# ---- the model on the stand-in --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", seq.FIXTURES)
def test_model_on_the_stand_in(name):
    """The sequence meets the fixture's tolerance, hn_* are the bits of update_posterior, the p_* attributes hold the
    traces, p_m_vec / p_nu / p_v_mat describe the next point, and the model's own row loop meets the same bound."""
    g = load_golden(name)
    x, start, exact, ref = seq.fixture_parts(g)
    n, D = x.shape
    m = seq.model_at(D, start)
    means, nats = m.pred_and_update_sequence(x, code_length=True)
    assert isinstance(means, np.ndarray) and means.dtype == np.float64 and means.shape == (n, D) and nats.shape == (n,)
    assert means is m.p_m_vecs and m.p_v_logdets.shape == m.p_quads.shape == m.p_nus.shape == (n,)
    assert np.array_equal(m.p_nus, g["ref_p_nu"])
    got = (m.p_m_vecs, m.p_v_logdets, m.p_quads, nats)
    print("worst error / tolerance: %.2f" % seq.check(name, got, exact, ref, x, D))
    u = seq.model_at(D, start).update_posterior(x)
    assert seq.hn_equal(m, u)
    assert np.allclose(m.hn_w_mat_inv, g["hn_w_mat_inv"], rtol=1e-9, atol=1e-12) and m.hn_kappa == float(g["hn_kappa"])
    u.calc_pred_dist()
    assert np.array_equal(m.p_m_vec, u.p_m_vec) and m.p_nu == u.p_nu and np.array_equal(m.p_v_mat, u.p_v_mat)
    # the model's own loop: what the sequence replaces
    lm = seq.model_at(D, start)
    loop = ([], [], [])
    for xi in x:
        pm = lm.pred_and_update(xi).copy()
        diff = xi - pm
        loop[0].append(pm)
        loop[1].append(np.linalg.slogdet(lm.p_v_mat)[1])
        loop[2].append(diff @ lm.p_v_mat @ diff)
    seq.check(name + " (the model's loop)", (np.array(loop[0]), np.array(loop[1]), np.array(loop[2]), nats), exact, ref, x, D)
    assert np.allclose(lm.hn_w_mat_inv, m.hn_w_mat_inv, rtol=1e-9, atol=1e-12)


def small_case(as_torch, dtype, D=3, n=40):
    x = (2.0 + np.random.default_rng(7).standard_normal((n, D))).astype(dtype)
    return seq.model_at(D, None), (torch.from_numpy(x) if as_torch else x)


@pytest.mark.parametrize("as_torch", (False, True))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_return_types_for_every_loss(as_torch, dtype):
    from bayesml_amd._exceptions import CriteriaError
    want = torch.Tensor if as_torch else np.ndarray
    n, D = 40, 3
    base = None
    for loss in ("squared", "0-1", None):
        for code_length in (False, True):
            m, x = small_case(as_torch, dtype)
            if loss is None and not code_length:
                with pytest.raises(CriteriaError, match="code_length=True"):
                    m.pred_and_update_sequence(x, loss=loss)
                continue
            out = m.pred_and_update_sequence(x, loss=loss, code_length=code_length)
            means, nats = out if (code_length and loss is not None) else ((None, out) if loss is None else (out, None))
            if loss is not None and code_length:
                assert isinstance(out, tuple) and len(out) == 2
            if nats is not None:
                assert isinstance(nats, want) and tuple(nats.shape) == (n,) and nats.dtype in (np.float64, torch.float64)
            if loss is None:
                assert m.p_m_vecs is None
            else:
                assert isinstance(means, want) and tuple(means.shape) == (n, D) and means.dtype in (np.float64, torch.float64)
                assert np.array_equal(np.asarray(means), m.p_m_vecs)
            assert m.p_v_logdets.shape == m.p_quads.shape == m.p_nus.shape == (n,)
            assert np.array_equal(m.p_nus, 3.0 + np.arange(n) - D + 1)
            if base is None:
                base = (m.p_v_logdets.copy(), m.p_quads.copy(), m.hn_m_vec.copy(), m.hn_w_mat_inv.copy())
            assert np.array_equal(m.p_v_logdets, base[0]) and np.array_equal(m.p_quads, base[1])
            assert np.array_equal(m.hn_m_vec, base[2]) and np.array_equal(m.hn_w_mat_inv, base[3])


def test_kl_and_bad_losses():
    from bayesml_amd._exceptions import CriteriaError
    m, x = small_case(False, np.float64)
    before = pickle.dumps(m)
    with pytest.raises(CriteriaError, match="multivariate_t cannot hold n parameter sets.*p_m_vecs, p_nus, p_v_logdets and p_quads"):
        m.pred_and_update_sequence(x, loss="KL")
    with pytest.raises(CriteriaError, match="multivariate_t"):
        m.pred_and_update_sequence(x, loss="KL", code_length=True)
    for bad in ("abs", "l2", 0, "kl"):
        with pytest.raises(CriteriaError, match="Unsupported loss function"):
            m.pred_and_update_sequence(x, loss=bad)
    assert pickle.dumps(m) == before


def test_a_refused_sample_changes_nothing():
    from bayesml_amd._exceptions import DataFormatError
    m, x = small_case(False, np.float64)
    m.pred_and_update_sequence(x)
    before = pickle.dumps(m)
    for bad in (x[:, :2], "x", np.array([["a", "b", "c"]]), torch.ones((4, 3), dtype=torch.int64), np.array(1.0)):
        with pytest.raises(DataFormatError):
            m.pred_and_update_sequence(bad)
    assert pickle.dumps(m) == before


def test_no_rows_is_no_work():
    m = seq.model_at(3, None)
    m._mvnseq_pass_factory = None             # nothing may be constructed, stand-in or engine
    m._data_pass_factory = None
    means, nats = m.pred_and_update_sequence(np.zeros((0, 3)), code_length=True)
    assert means.shape == (0, 3) and nats.shape == m.p_v_logdets.shape == m.p_quads.shape == m.p_nus.shape == (0,)
    assert m.hn_kappa == 1.0 and m.hn_nu == 3.0 and m._seq_engine is None
    assert m.pred_and_update_sequence(torch.zeros((0, 3)), loss=None, code_length=True).shape == (0,) and m.p_m_vecs is None


def test_loss_none_asks_for_no_means_and_dtypes_reach_the_engine_unchanged():
    seen = []

    def recording(D):
        seen.append(seq.CpuMvnSeqPass(D))
        return seen[-1]
    x = np.random.default_rng(5).standard_normal((9, 2))
    for dtype, tdtype in ((np.float32, torch.float32), (np.float64, torch.float64)):
        m = seq.model_at(2, None)
        m._mvnseq_pass_factory = recording
        full = m.pred_and_update_sequence(x.astype(dtype), code_length=True)[1]
        assert seen[-1].last_dtype == tdtype and seen[-1].last_want == ("means", "logdet", "quad", "nats")
        m = seq.model_at(2, None)
        m._mvnseq_pass_factory = recording
        alone = m.pred_and_update_sequence(x.astype(dtype), loss=None, code_length=True)
        assert seen[-1].last_want == ("logdet", "quad", "nats") and np.array_equal(full, alone)
    m = seq.model_at(2, None)
    view = torch.from_numpy(np.random.default_rng(6).standard_normal((9, 5)))[:, :2]
    m._mvnseq_pass_factory = recording
    strided = m.pred_and_update_sequence(view)
    assert np.array_equal(strided.numpy(), seq.model_at(2, None).pred_and_update_sequence(view.contiguous().numpy()))


def test_one_pass_against_several_through_the_model():
    x = 1.0 + np.random.default_rng(8).standard_normal((3 * B + 17, 4))
    outs = []
    for per in (None, 1, 3):
        m = seq.model_at(4, None)
        m._mvnseq_pass_factory = lambda D, per=per: seq.CpuMvnSeqPass(D, per)
        means, nats = m.pred_and_update_sequence(x, code_length=True)
        outs.append((means, nats, m.p_v_logdets, m.p_quads, m.hn_w_mat_inv))
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))


def test_pickle_round_trip():
    m, x = small_case(True, np.float64)
    m.pred_and_update_sequence(x)
    m._seq_engine = object()                    # whatever the engine is, it does not travel
    m._mvnseq_pass_factory = None
    m._data_pass_factory = None
    c = pickle.loads(pickle.dumps(m))
    assert c._seq_engine is None
    assert np.array_equal(c.p_m_vecs, m.p_m_vecs) and np.array_equal(c.p_quads, m.p_quads) and np.array_equal(c.p_nus, m.p_nus)
    assert np.array_equal(c.hn_w_mat_inv, m.hn_w_mat_inv) and c.p_v_logdets.shape == (40,)


def test_product_path_fails_loudly_without_a_gpu():
    if torch.cuda.is_available():
        return                                  # (an unmarked test does not touch the device)
    from bayesml_amd import multivariate_normal as mvn
    from bayesml_amd._engine import EngineLimitError, EngineUnavailableError
    m = mvn.LearnModel(2)
    with pytest.raises(EngineUnavailableError):
        m.pred_and_update_sequence(np.zeros((4, 2)))
    assert m.hn_kappa == 1.0 and m.p_v_logdets.shape == (0,)
    with pytest.raises(EngineLimitError):
        mvn.LearnModel(257).pred_and_update_sequence(np.zeros((4, 257)))
