"""contexttree.LearnModel.pred_and_update_sequence on the MI355X: the ctseq engine against the reference's fixtures, the
per-symbol loop, the NumPy restatement and the exact recursion."""
import copy
import functools
import math
import re

import numpy as np
import pytest
import torch

import contexttree_oracle as orc
import contexttree_seq_oracle as seq
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NAMES = [c["name"] for c in orc.CASES]
TRACE_RTOL = {"k3_d2": 6e-11, "k3_d3_long": 1.5e-12}      # test_gpu_contexttree.py's, for the trace from the posterior
LOOP_SHAPES = ((3, 3, 31, 2000), (2, 5, 32, 2000), (5, 4, 33, 2000), (256, 2, 34, 3000), (1, 2, 35, 2000))
STATES = ("fresh", "updated", "hn_changed")


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _ctseq():
    from bayesml_amd import _ctseq
    return _ctseq


def _prior(kind, k):
    return np.arange(1, k + 1) / 2.0 if kind == "dyadic" else 0.3 + 0.7 * np.sqrt(np.arange(1, k + 1))


def _tables(m):
    return m._eng().get_tables()


def _same_nodes(a, b):
    ex = a["exists"] != 0
    return (np.array_equal(a["exists"], b["exists"]) and np.array_equal(a["leaf"][ex], b["leaf"][ex])
            and np.array_equal(a["beta"][ex], b["beta"][ex]))


def _bytes_for(k, D, m, want_rows=False):
    return 8 * _ctseq().work_slots(k, D, m, want_rows)


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reference_traces(name):
    """Both 50-step traces of every fixture.  From the prior: test_gpu_contexttree.py's bounds, h_g by trace_g_ok(tol=0).
    From the posterior: its bounds on the probabilities; the h_g the trace leaves are held by trace_g_ok from starts
    4 x ref_vs_batch + 64 eps apart in log-odds (the posterior's own bound there).  A log-odds bound on the END state
    cannot hold for this form: k2_d3 has a node with 1 - h_g = 7e-14, where one ulp of h_g is 1.5e-3 in log-odds, and the
    reference rounds h_g once per step while the prefix sum carries the log-odds - the two differ by such ulps."""
    ct = _ct()
    case, fx = orc.case_by_name(name), load_golden(f"contexttree_{name}.npz")
    inp, k, D = orc.case_inputs(case), case["k"], case["D"]
    h0_root = ct.GenModel(k, D, h_g=0.8, seed=case["seed"]).gen_params().root if case["h0root"] else None
    m = ct.LearnModel(k, D, case["h0_g"], np.arange(1, k + 1) / 2.0, h0_root)
    tr = inp["trace_x"]

    m0 = copy.deepcopy(m)
    p0 = m0.pred_and_update_sequence(tr)
    t0 = orc.tree_to_tables(m0.hn_root, k, D)
    np.testing.assert_allclose(p0, fx["trace0_p"], rtol=1e-12, atol=0)
    assert np.array_equal(p0.argmax(1), fx["trace0_p"].argmax(1))
    assert np.array_equal(m0.p_theta_vec, p0[-1])
    assert np.array_equal(t0["exists"], fx["trace0_exists"]) and np.array_equal(t0["leaf"], fx["trace0_leaf"])
    assert np.array_equal(t0["beta"], fx["trace0_beta"])
    assert orc.trace_g_ok(t0["g"], fx["trace0_g"], fx["trace0_exists"], tol=0)

    m.update_posterior(inp["x1"])
    if case["hn2"] is not None:
        m.set_hn_params(case["hn2"][0], np.array(case["hn2"][1]))
    if len(inp["x2"]):
        m.update_posterior(inp["x2"])
    p, nats = m.pred_and_update_sequence(tr, code_length=True)
    t = orc.tree_to_tables(m.hn_root, k, D)
    tol = 4 * float(fx["ref_vs_batch"]) + 64 * EPS
    rel = float(np.max(np.abs(p - fx["trace_p"]) / fx["trace_p"]))
    print(f"{name} sequence trace: relative error {rel:.3e}")
    assert np.array_equal(p.argmax(1), fx["trace_p"].argmax(1))
    assert np.array_equal(t["exists"], fx["final_exists"]) and np.array_equal(t["leaf"], fx["final_leaf"])
    assert np.array_equal(t["beta"], fx["final_beta"])
    assert orc.trace_g_ok(t["g"], fx["final_g"], fx["final_exists"], tol)
    np.testing.assert_allclose(p, fx["trace_p"], rtol=TRACE_RTOL.get(name, 1e-12), atol=0)
    np.testing.assert_allclose(nats, -np.log(fx["trace_p"][np.arange(len(tr)), tr]), rtol=0,
                               atol=TRACE_RTOL.get(name, 1e-12) + 4 * EPS * np.max(nats))


# ---- 2. the per-symbol loop ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sample(k, seed, n):
    return orc.planted_sample(k, n, np.random.default_rng(seed))


def _start(k, D, seed, state, prior):
    m = _ct().LearnModel(k, D, 0.5, _prior(prior, k))
    if state == "updated":
        m.update_posterior(_sample(k, seed + 100, 1000))
    if state == "hn_changed":                # the nodes that the sequence creates read the changed defaults
        m.set_hn_params(0.35, _prior(prior, k)[::-1].copy())
    return m


@functools.lru_cache(maxsize=None)
def _loop(k, D, seed, n, state, prior):
    """The per-symbol loop, run once per start and shared (results are not modified)."""
    m, x = _start(k, D, seed, state, prior), _sample(k, seed, n)
    p = np.stack([m.pred_and_update(x[:i + 1]).copy() for i in range(n)])
    return p, _tables(m), m.p_theta_vec.copy()


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("k,D,seed,n", LOOP_SHAPES)
def test_against_the_loop_dyadic(k, D, seed, n, state):
    p_ref, t_ref, last = _loop(k, D, seed, n, state, "dyadic")
    m, x = _start(k, D, seed, state, "dyadic"), _sample(k, seed, n)
    p, nats = m.pred_and_update_sequence(x, code_length=True)
    t = _tables(m)
    atol = orc.trace_p_atol(0, D, steps=n)
    print(f"k={k} D={D} {state}: max |dP| {np.abs(p - p_ref).max():.3e}, bound {atol:.3e}")
    assert p.shape == (n, k) and p.dtype == np.float64 and nats.shape == (n,)
    assert _same_nodes(t_ref, t)
    assert np.max(np.abs(p - p_ref)) <= atol
    assert orc.trace_g_ok(t["g"], t_ref["g"], t_ref["exists"], tol=0, steps=n)
    assert np.array_equal(m.p_theta_vec, p[-1])
    q = p_ref[np.arange(n), x]
    assert np.max(np.abs(nats + np.log(q)) * q) <= atol + 4 * EPS * np.max(nats * q + 1)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("k,D,seed,n", LOOP_SHAPES)
def test_against_the_loop_argmax(k, D, seed, n, state):
    p_ref, t_ref, last = _loop(k, D, seed, n, state, "sqrt")
    x = _sample(k, seed, n)
    m = _start(k, D, seed, state, "sqrt")
    p = m.pred_and_update_sequence(x)
    assert np.max(np.abs(p - p_ref)) <= orc.trace_p_atol(0, D, steps=n)
    m = _start(k, D, seed, state, "sqrt")
    am = m.pred_and_update_sequence(x, loss="0-1")
    assert am.dtype == np.int64 and am.shape == (n,)
    assert np.array_equal(am, p_ref.argmax(1))
    assert np.max(np.abs(m.p_theta_vec - last)) <= orc.trace_p_atol(0, D, steps=n)


# ---- 3. the exact recursion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g0", [0.5, 1 - 2.0 ** -20, 2.0 ** -30, 0.0, 1.0])
@pytest.mark.parametrize("k,D", [(2, 4), (3, 3)])
def test_exact_oracle(k, D, g0):
    mp = orc._mp()
    n, prior = 600, np.arange(1, k + 1) / 2.0
    x = orc.planted_sample(k, n, np.random.default_rng(40 + k))
    exact = seq.sequence_exact(x, k, D, orc.new_tables(k, D), g0, prior)
    m = _ct().LearnModel(k, D, g0, prior)
    p, nats = m.pred_and_update_sequence(x, code_length=True)
    t = _tables(m)
    assert np.array_equal(t["exists"], exact["exists"])
    worst_g = worst_p = 0.0
    for i in np.flatnonzero(exact["exists"]):
        ge = exact["g"][i]
        if exact["logit"][i] is None:
            assert t["g"][i] == float(ge), i          # 0 and 1 are fixed points, bit for bit
            continue
        err, bound = abs(mp.mpf(float(t["g"][i])) - ge), orc.g_bound(ge, exact["B"][i])
        worst_g = max(worst_g, float(err / bound))
        assert err <= bound, (i, float(err), float(bound))
    for i in range(n):
        bound = exact["p_bound"][i] + 8 * (D + 1) * EPS
        for a in range(k):
            err = abs(mp.mpf(float(p[i, a])) - exact["p"][i][a])
            worst_p = max(worst_p, float(err / bound))
            assert err <= bound, (i, a, float(err), float(bound))
        pe = exact["p"][i][int(x[i])]
        assert abs(mp.mpf(float(nats[i])) + mp.log(pe)) <= bound / pe + 2 * EPS * abs(mp.log(pe)), i
    print(f"k={k} D={D} g0={g0}: worst error / bound: h_g {worst_g:.3f}, rows {worst_p:.3f}")
    if g0 in (0.0, 1.0):
        # g0 = 0: every row is the root's own estimate; g0 = 1: the own estimate of the path's end
        rows, _ = seq.sequence(x, k, D, orc.new_tables(k, D), g0, prior)
        assert np.array_equal(p, rows)


# ---- 4. chunks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_len", [1, 7, 64, 65, 4097])
@pytest.mark.parametrize("k,D", [(2, 6), (4, 3)])
def test_chunks(k, D, m_len):
    from bayesml_amd import _ctree
    cs = _ctseq()
    n, prior = 4100, np.arange(1, k + 1) / 2.0
    x = orc.planted_sample(k, n, np.random.default_rng(50 + k))
    assert cs.plan_chunks(n, k, D, False, _bytes_for(k, D, m_len)) == m_len

    one = _ct().LearnModel(k, D, 0.5, prior)
    p_one = one.pred_and_update_sequence(x)
    cut = _ct().LearnModel(k, D, 0.5, prior)
    p_cut, nats_cut = cut.pred_and_update_sequence(x, code_length=True, chunk_bytes=_bytes_for(k, D, m_len))
    assert cut._seq_pass.passes == math.ceil(n / m_len)
    t_one, t_cut = _tables(one), _tables(cut)
    assert _same_nodes(t_one, t_cut)
    assert np.max(np.abs(p_one - p_cut)) <= 2 * orc.trace_p_atol(0, D, steps=n)
    assert orc.trace_g_ok(t_cut["g"], t_one["g"], t_one["exists"], tol=0, steps=n)

    # explicit calls of the entry point on the same pieces: bit for bit
    dev = torch.device("cuda", 0)
    eng = _ctree.CtreePass(k, D, dev)
    lib = cs.load_library()
    xd = torch.from_numpy(x).to(dev)
    hb = torch.from_numpy(prior).to(dev)
    rows = torch.empty(n, k, dtype=torch.float64, device=dev)
    nats = torch.empty(n, dtype=torch.float64, device=dev)
    for b in range(0, n, m_len):
        mm = min(m_len, n - b)
        work = torch.empty(int(lib.ctseq_work_len(k, D, mm, 0)), dtype=torch.int64, device=dev)
        rc = lib.ctseq_pass(_ctree.I64, xd.data_ptr(), n, b, mm, k, D, eng.beta.data_ptr(), eng.g.data_ptr(),
                            eng.exists.data_ptr(), eng.leaf.data_ptr(), 0.5, hb.data_ptr(), rows[b:].data_ptr(), None,
                            nats[b:].data_ptr(), work.data_ptr(), None)
        assert rc == 0, lib.ctseq_last_error()
    torch.cuda.synchronize()
    t_exp = eng.get_tables()
    ex = t_exp["exists"] != 0
    assert np.array_equal(rows.cpu().numpy(), p_cut) and np.array_equal(nats.cpu().numpy(), nats_cut)
    assert _same_nodes(t_exp, t_cut) and np.array_equal(t_exp["g"][ex], t_cut["g"][ex])


# ---- 5. long and short segments -----------------------------------------------------------------------------------------
def _edges_sample(n, rng):
    """k and a sample whose level-1 segments (and level-0 symbol runs) start at, just before and just after every multiple
    of the row block (64), hence of the tile (256) and of the scan workgroup (1024): run lengths 63, 1, 1, 62, 1, 1, 62..."""
    lens = [63, 1, 1]
    while sum(lens) < n - 1:
        lens += [62, 1, 1]
    k = len(lens)
    body = np.repeat(np.arange(k), lens)[:n - 1]
    return k, np.append(rng.permutation(body), 0)


@pytest.mark.parametrize("kind", ["all_equal_k2", "all_equal_k5", "edges"])
def test_long_and_short_segments(kind):
    cs = _ctseq()
    assert (cs.TILE, cs.ROW_BLOCK) == (256, 64)
    n = 3 * 1024 + 17                       # 1024: the workgroup of the two single-workgroup scans, the largest constant
    rng = np.random.default_rng(60)
    if kind == "edges":
        (k, x), D = _edges_sample(n, rng), 2
        starts = np.concatenate([[0], np.cumsum(np.bincount(x[:n - 1], minlength=k))])
        for c in range(64, n - 64, 64):
            assert {c - 1, c, c + 1} <= set(starts.tolist()), c
    else:
        k, D = int(kind[-1]), 6 if kind.endswith("2") else 3
        x = np.full(n, k - 1, dtype=np.int64)
    prior = np.arange(1, k + 1) / 2.0
    t = orc.new_tables(k, D)
    rows, nats = seq.sequence(x, k, D, t, 0.5, prior)
    m = _ct().LearnModel(k, D, 0.5, prior)
    p, got_nats = m.pred_and_update_sequence(x, code_length=True)
    am = _ct().LearnModel(k, D, 0.5, prior).pred_and_update_sequence(x, loss="0-1")
    got = _tables(m)
    atol = orc.trace_p_atol(0, D, steps=n)
    print(f"{kind}: max |dP| {np.abs(p - rows).max():.3e}, bound {atol:.3e}")
    assert _same_nodes(t, got)
    assert np.max(np.abs(p - rows)) <= atol
    assert orc.trace_g_ok(got["g"], t["g"], t["exists"], tol=0, steps=n)
    q = np.exp(-nats)
    assert np.max(np.abs(got_nats - nats) * q) <= atol + 4 * EPS * np.max(nats * q + 1)
    clear = np.sort(rows, axis=1)[:, -1] - (np.sort(rows, axis=1)[:, -2] if k > 1 else 0) > 2 * atol
    assert np.array_equal(am[clear], rows.argmax(1)[clear])


def test_more_tiles_than_scan_threads():
    """m above 1024 tiles of 256: each thread of the single-workgroup scans then folds several tiles, and with four
    nodes at the deepest level every segment runs through hundreds of tiles.  No rows: the scalar pass alone."""
    k, D = 2, 2
    n = 1024 * 256 + 3 * 1024 + 17
    x = np.random.default_rng(61).choice(k, n, p=[0.8, 0.2])
    prior = np.arange(1, k + 1) / 2.0
    t = orc.new_tables(k, D)
    _, nats = seq.sequence(x, k, D, t, 0.5, prior, want_rows=False)
    m = _ct().LearnModel(k, D, 0.5, prior)
    got_nats = m.pred_and_update_sequence(x, loss=None, code_length=True)
    assert m._seq_pass.passes == 1
    got = _tables(m)
    atol = orc.trace_p_atol(0, D, steps=n)
    q = np.exp(-nats)
    print(f"n={n}: max |dq| {np.max(np.abs(got_nats - nats) * q):.3e}, bound {atol:.3e}")
    assert _same_nodes(t, got)
    assert np.max(np.abs(got_nats - nats) * q) <= atol + 4 * EPS * np.max(nats * q + 1)
    assert orc.trace_g_ok(got["g"], t["g"], t["exists"], tol=0, steps=n)


# ---- 6. dtypes and views ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,D", [(2, 6), (5, 3)])
def test_dtypes_and_views(k, D):
    n, rng = 1500, np.random.default_rng(70)
    prior = np.arange(1, k + 1) / 2.0
    big = rng.integers(0, k, n + 3)
    want = {}
    for start in range(4):
        x = big[start:start + n]
        want[start] = _ct().LearnModel(k, D, 0.5, prior).pred_and_update_sequence(x, code_length=True)
        assert np.max(np.abs(want[start][0].sum(1) - 1)) <= 4 * k * EPS
    for dt in (torch.uint8, torch.int32, torch.int64):
        buf = torch.from_numpy(big).to(dt).cuda()
        for start in range(4):
            m = _ct().LearnModel(k, D, 0.5, prior)
            p, nats = m.pred_and_update_sequence(buf[start:start + n], code_length=True)
            assert isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float64 and p.shape == (n, k)
            assert isinstance(nats, torch.Tensor) and nats.is_cuda and nats.shape == (n,)
            assert np.array_equal(p.cpu().numpy(), want[start][0]) and np.array_equal(nats.cpu().numpy(), want[start][1])
    am = _ct().LearnModel(k, D, 0.5, prior).pred_and_update_sequence(torch.from_numpy(big[:n]).cuda(), loss="0-1")
    assert isinstance(am, torch.Tensor) and am.is_cuda and am.dtype == torch.int64
    only = _ct().LearnModel(k, D, 0.5, prior).pred_and_update_sequence(big[:n], loss=None, code_length=True)
    assert isinstance(only, np.ndarray) and np.array_equal(only, want[0][1])


# ---- 7. bad symbols -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "cut"])
@pytest.mark.parametrize("value", [-1, "k", 255])
def test_bad_symbols_change_nothing(where, value):
    from bayesml_amd._exceptions import DataFormatError
    from bayesml_amd import _check
    k, D, n, m_len = 3, 3, 500, 64
    rng = np.random.default_rng(80)
    m = _ct().LearnModel(k, D, 0.5, np.arange(1, k + 1) / 2.0)
    m.pred_and_update_sequence(rng.integers(0, k, 300))
    before, p_before = _tables(m), m.p_theta_vec.copy()
    x = rng.integers(0, k, n)
    x[{"first": 0, "last": n - 1, "cut": m_len}[where]] = k if value == "k" else value
    text = "x" + _check.SAMPLE_MSG["nonneg_ints"] if value == -1 else f"x.max() must smaller than c_k:{k}"
    with pytest.raises(DataFormatError) as info:
        m.pred_and_update_sequence(x, chunk_bytes=_bytes_for(k, D, m_len))
    assert str(getattr(info.value, "value", info.value)) == text
    after = _tables(m)
    for name in ("g", "beta", "exists", "leaf"):
        assert np.array_equal(before[name], after[name]), name
    assert np.array_equal(p_before, m.p_theta_vec)


# ---- 8. determinism -----------------------------------------------------------------------------------------------------
def test_two_runs_are_equal():
    k, D, n = 4, 5, 20011
    x = torch.from_numpy(orc.planted_sample(k, n, np.random.default_rng(90))).cuda()
    runs = []
    for _ in range(2):
        m = _ct().LearnModel(k, D, 0.5, 0.3 + 0.7 * np.sqrt(np.arange(1, k + 1)))
        p, nats = m.pred_and_update_sequence(x, code_length=True, chunk_bytes=_bytes_for(k, D, 7001))
        e = m._eng()
        runs.append((p, nats, e.g.clone(), e.beta.clone(), e.exists.clone(), e.leaf.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 9. the end state against update_posterior --------------------------------------------------------------------------
@pytest.mark.parametrize("k,D", [(2, 10), (4, 6)])
def test_end_state_is_update_posterior_s(k, D):
    n, prior = 200003, np.arange(1, k + 1) / 2.0
    x = torch.from_numpy(np.random.default_rng(95).integers(0, k, n)).cuda()
    a = _ct().LearnModel(k, D, 0.5, prior).update_posterior(x)
    b = _ct().LearnModel(k, D, 0.5, prior)
    budget, p_before = 8 << 20, b.p_theta_vec.copy()
    nats = b.pred_and_update_sequence(x, loss=None, code_length=True, chunk_bytes=budget)
    m_len = _ctseq().plan_chunks(n, k, D, False, budget)
    assert 1 < math.ceil(n / m_len) == int(re.search(r"x (\d+) ", b._seq_pass.launch_info).group(1))
    assert _same_nodes(_tables(a), _tables(b))
    assert isinstance(nats, torch.Tensor) and nats.shape == (n,)
    assert bool(torch.isfinite(nats).all()) and bool((nats > 0).all())
    assert np.array_equal(b.p_theta_vec, p_before)               # loss=None leaves p_theta_vec alone
