"""contexttree on the MI355X: ctree_count / ctree_sweep / ctree_map against NumPy and against the reference's fixtures."""
import warnings

import numpy as np
import pytest
import torch

import contexttree_oracle as orc
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NAMES = [c["name"] for c in orc.CASES]
TORCH_DT = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
LENGTHS = (1, 2, None, None, 63, 64, 65, 257, 4097, 100003)       # None: D and D + 1
# both sides of the LDS / global table boundary (k^(D+1) <= 4096 | > 4096), the widest alphabet and the smallest tree
SHAPES = ((2, 11), (2, 12), (4, 5), (4, 6), (3, 7), (256, 1), (2, 1))


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _pass(k, D):
    from bayesml_amd import _ctree
    return _ctree.CtreePass(k, D, torch.device("cuda", 0))


def _skewed(k, n, rng):
    """Independent symbols with very unequal probabilities: a few hot contexts and many rare ones."""
    return rng.choice(k, n, p=rng.dirichlet(np.ones(k) * 0.3))


def _all_level_counts(eng, x):
    """[cnt_0, ..., cnt_D] of the device tensor x through ctree_count + ctree_sweep's optional output, and (n, bad)."""
    out = eng.count(x)
    n, bad = (int(v) for v in out[:2].cpu())
    deepest = out[2:].clone()
    eng.clear()
    upper = eng.sweep(x, 0.5, np.ones(eng.k) / 2, want_counts=True).cpu().numpy()
    levels = [upper[eng.off[d]:eng.off[d + 1]] for d in range(eng.D)]
    return levels + [deepest.cpu().numpy().reshape(-1, eng.k)], n, bad


def _check_counts(eng, x_np, x_dev):
    got, n, bad = _all_level_counts(eng, x_dev)
    want = orc.level_counts(x_np, eng.k, eng.D)
    assert (n, bad) == (len(x_np), 0)
    for d in range(eng.D + 1):
        assert np.array_equal(got[d], want[d]), (eng.k, eng.D, len(x_np), d)


@pytest.mark.parametrize("k,D", [(3, 4), (2, 12)])
def test_counts_every_length(k, D):
    eng, rng = _pass(k, D), np.random.default_rng(k * 100 + D)
    for n in LENGTHS[:2] + (D, D + 1) + LENGTHS[4:]:
        x = rng.integers(0, k, n)
        _check_counts(eng, x, torch.from_numpy(x).cuda())


@pytest.mark.parametrize("k,D", [(2, 11), (4, 6)])
def test_counts_dtypes_and_views(k, D):
    eng, rng = _pass(k, D), np.random.default_rng(7)
    for name, dt in TORCH_DT.items():
        for start in range(4):
            x = rng.integers(0, k, 4097 + 3)
            buf = torch.from_numpy(x).to(dt).cuda()
            _check_counts(eng, x[start:start + 4097], buf[start:start + 4097])


@pytest.mark.parametrize("k,D", SHAPES)
def test_counts_every_shape(k, D):
    eng, rng = _pass(k, D), np.random.default_rng(k + D)
    x = _skewed(k, 20011, rng)
    _check_counts(eng, x, torch.from_numpy(x).to(torch.int32).cuda())
    x = rng.integers(0, k, 100003)
    _check_counts(eng, x, torch.from_numpy(x).to(torch.uint8 if k <= 255 else torch.int32).cuda())


def test_counts_largest_table():
    """(2, 23): 2^24 slots, compared on the device (the sparse expectation is built by index_put)."""
    k, D, n = 2, 23, 4097
    eng, rng = _pass(k, D), np.random.default_rng(23)
    x = rng.integers(0, k, n)
    out = eng.count(torch.from_numpy(x).to(torch.uint8).cuda())
    want = orc.level_counts(x, k, D)
    assert [int(v) for v in out[:2].cpu()] == [n, 0]
    idx = np.flatnonzero(want[D].reshape(-1))
    exp = torch.zeros(k ** (D + 1), dtype=torch.int64, device="cuda")
    exp[torch.from_numpy(idx).cuda()] = torch.from_numpy(want[D].reshape(-1)[idx]).cuda()
    assert torch.equal(out[2:], exp) and int(exp.sum()) == n - D
    eng.clear()
    upper = eng.sweep(torch.from_numpy(x).cuda(), 0.5, np.ones(k) / 2, want_counts=True)
    for d in (0, 1, 7, D - 1):
        assert np.array_equal(upper[eng.off[d]:eng.off[d + 1]].cpu().numpy(), want[d]), d
    assert int(eng.exists.sum()) == sum(int((want[d].sum(1) > 0).sum()) for d in range(D + 1))


@pytest.mark.parametrize("k,D", [(2, 5), (2, 12)])
def test_counts_hot_bin_and_range_boundaries(k, D):
    """All-equal symbols (every add of a workgroup hits one bin), and a pattern planted across every workgroup range
    boundary, at a length whose ranges are 4096 samples and at one whose ranges are not a multiple of anything (4883)."""
    eng = _pass(k, D)
    for n, span in ((100003, 4096), (5000000, 4883)):
        assert max(4096, -(-n // 1024)) == span
        x = np.ones(n, dtype=np.int64)
        _check_counts(eng, x, torch.from_numpy(x).to(torch.uint8).cuda())
        x = np.zeros(n, dtype=np.int64)
        for b in range(span, n, span):
            x[b - 2:b + 2] = (1, 0, 1, 1)
        _check_counts(eng, x, torch.from_numpy(x).to(torch.uint8).cuda())


@pytest.mark.parametrize("dtype,bad_value", [("i64", -1), ("i32", 2), ("u8", 255), ("u8", 2)])
@pytest.mark.parametrize("k,D", [(2, 5), (2, 12)])
def test_bad_symbols(k, D, dtype, bad_value):
    """bad is exact, the windows with a bad symbol are dropped and nothing else moves; the model refuses the sample and
    keeps its state."""
    ct = _ct()
    eng, rng = _pass(k, D), np.random.default_rng(3)
    n = 3 * 4096 + 17
    clean = rng.integers(0, k, n)
    for places in ([0], [n - 1], [4095], [4096], [0, 4096, 4097, n - 1]):
        x = clean.copy()
        x[places] = bad_value
        out = eng.count(torch.from_numpy(x).to(TORCH_DT[dtype]).cuda())
        bad, want = orc.deepest_counts(x, k, D)
        assert [int(v) for v in out[:2].cpu()] == [n, len(places)] and bad == len(places)
        assert np.array_equal(out[2:].cpu().numpy().reshape(-1, k), want)
    m = ct.LearnModel(k, D, device="cuda:0")
    m.update_posterior(clean[:500])
    e = m._eng()
    before = [t.clone() for t in (e.g, e.beta, e.exists, e.leaf)]
    with pytest.raises(ct._contexttree.DataFormatError) as err:
        m.update_posterior(torch.from_numpy(x).to(TORCH_DT[dtype]).cuda())
    msg = ("x must be int or a numpy.ndarray whose dtype is int. Its values must be non-negative (including 0)."
           if bad_value < 0 else f"x.max() must smaller than c_k:{k}")
    assert err.value.value == msg
    assert all(torch.equal(a, b) for a, b in zip(before, (e.g, e.beta, e.exists, e.leaf)))


def test_untouched_nodes_keep_their_bits():
    """Entries of nodes without samples are not written at all: sentinels survive, existing or not."""
    k, D = 3, 4
    eng, rng = _pass(k, D), np.random.default_rng(5)
    x = orc.planted_sample(k, 300, rng)
    cnt = orc.level_counts(x, k, D)
    untouched = np.concatenate([c.sum(1) == 0 for c in cnt])
    assert untouched.sum() > 20
    exists = (rng.random(eng.nodes) < 0.5).astype(np.uint8)
    exists[0] = 1
    g = rng.random(eng.nodes)
    g[eng.off[D]:] = 0.0
    beta = rng.random((eng.nodes, k)) + 0.5
    eng.set_tables(dict(g=g, beta=beta, exists=exists, leaf=np.zeros(eng.nodes, np.uint8)))
    eng.update(torch.from_numpy(x).cuda(), 0.4, np.array([1.0, 2.0, 3.0]))
    t = eng.get_tables()
    assert np.array_equal(t["g"][untouched], g[untouched]) and np.array_equal(t["beta"][untouched], beta[untouched])
    assert np.array_equal(t["exists"][untouched], exists[untouched]) and np.all(t["exists"][~untouched] == 1)
    # and the touched ones follow the oracle from the same tables
    want = dict(g=g.copy(), beta=beta.copy(), exists=exists.copy(), leaf=np.zeros(eng.nodes, np.uint8))
    orc.batch_update(x, k, D, want, 0.4, np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(t["beta"], want["beta"]) and np.array_equal(t["exists"], want["exists"])
    assert orc.log_odds_err(t["g"], want["g"], want["exists"]) < 1e-9


def test_two_runs_are_bitwise_equal():
    ct, rng = _ct(), np.random.default_rng(9)
    for k, D, n in ((2, 10, 200003), (4, 6, 200003)):          # the LDS path and the global-atomic path
        x = torch.from_numpy(_skewed(k, n, rng)).cuda()
        runs = []
        for _ in range(2):
            m = ct.LearnModel(k, D, device="cuda:0").update_posterior(x)
            runs.append(m._eng())
        for name in ("g", "beta", "exists", "leaf"):
            assert torch.equal(getattr(runs[0], name), getattr(runs[1], name)), (k, D, name)


@pytest.fixture(scope="module")
def driven():
    """Every fixture case walked through the drop-in on the GPU, once."""
    ct = _ct()
    make = lambda *a: ct.LearnModel(*a, device="cuda:0")          # noqa: E731
    res = {}
    for case in orc.CASES:
        res[case["name"]] = orc.drive(ct, case, orc.case_inputs(case), make=make)[0]
    return res


@pytest.mark.parametrize("name", NAMES)
def test_posterior_parity(name, driven):
    """h_beta_vec, the node set and the leaf flags exactly; h_g in log-odds to 4 x ref_vs_batch + 64 eps of the case (the
    device differs from the oracle by its lgamma and the order of the child sums: errors of the kind and size of the
    oracle's own against the reference)."""
    case, out, fx = orc.case_by_name(name), driven[name], load_golden(f"contexttree_{name}.npz")
    tol = 4 * float(fx["ref_vs_batch"]) + 64 * EPS
    for stage in ("after1", "after2"):
        if f"{stage}_exists" not in fx:
            assert f"{stage}_exists" not in out
            continue
        ex = fx[f"{stage}_exists"]
        assert np.array_equal(out[f"{stage}_exists"], ex)
        assert np.array_equal(out[f"{stage}_beta"], fx[f"{stage}_beta"])
        assert np.array_equal(out[f"{stage}_leaf"], fx[f"{stage}_leaf"])
        err = orc.log_odds_err(out[f"{stage}_g"], fx[f"{stage}_g"], ex)
        print(f"{name} {stage}: log-odds error {err:.3e}, bound {tol:.3e}")
        assert err <= tol


@pytest.mark.parametrize("name", NAMES)
def test_prior_nodes_without_samples_are_bit_identical(name, driven):
    case, out = orc.case_by_name(name), driven[name]
    prior = orc.prior_tables(_ct(), case)
    cnt = orc.level_counts(orc.case_inputs(case)["x1"], case["k"], case["D"])
    keep = np.concatenate([c.sum(1) == 0 for c in cnt]) & (prior["exists"] != 0)
    assert np.array_equal(out["after1_g"][keep], prior["g"][keep])
    assert np.array_equal(out["after1_beta"][keep], prior["beta"][keep])
    assert np.array_equal(out["after1_leaf"][keep], prior["leaf"][keep])
    if case["h0root"]:
        assert keep.sum() > 0


@pytest.mark.parametrize("name", NAMES)
def test_map_tree(name, driven):
    out, fx = driven[name], load_golden(f"contexttree_{name}.npz")
    assert np.array_equal(out["map_in_tree"], fx["map_in_tree"]) and np.array_equal(out["map_leaf"], fx["map_leaf"])
    assert np.array_equal(np.isnan(out["map_theta"]), np.isnan(fx["map_theta"]))
    np.testing.assert_allclose(np.nan_to_num(out["map_theta"]), np.nan_to_num(fx["map_theta"]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_pred_dist(name, driven):
    """calc_pred_dist on three contexts (one shorter than c_d_max): probabilities to 1e-12 relative, argmax and the nodes
    that the call creates exactly.

    The case that decides is k3_d3_long (N = 1e5): a node's log-odds are a difference of log-likelihoods of the size of N,
    so lnDM has to be evaluated without the cancellation of lgamma values of the size of N ln N
    (ctree_kernels.h: dm_row_and_update); by lgamma alone this case is 1.4e-12 off."""
    out, fx = driven[name], load_golden(f"contexttree_{name}.npz")
    for j in range(3):
        rel = np.max(np.abs(out[f"pred{j}"] - fx[f"pred{j}"]) / fx[f"pred{j}"])
        print(f"{name} pred{j}: relative error {rel:.3e}")
        assert out[f"pred{j}_argmax"] == fx[f"pred{j}_argmax"]
        assert np.array_equal(out[f"pred{j}_exists"], fx[f"pred{j}_exists"])
    for j in range(3):
        np.testing.assert_allclose(out[f"pred{j}"], fx[f"pred{j}"], rtol=1e-12, atol=0)


# Cases whose trace from the posterior cannot meet 1e-12 relative: the measured value on an MI355X and a bound just above it
# (reasons in test_pred_and_update_trace's docstring).
TRACE_RTOL = {"k3_d2": 6e-11, "k3_d3_long": 1.5e-12}


@pytest.mark.parametrize("name", NAMES)
def test_pred_and_update_trace(name, driven):
    """The 50-step pred_and_update trace that starts from the posterior the kernels produced: probabilities to 1e-12
    relative, argmax, node set, leaf flags and h_beta_vec exactly, and the h_g it leaves in log-odds to the posterior's own
    bound, 4 x ref_vs_batch + 64 eps.  (A second trace, from the prior, checks the gather and scatter of rows alone.)

    Two cases need more than 1e-12; measured on an MI355X:
    * k3_d2: 4.7e-11.  After 500 symbols one node has 1 - h_g = 1.6e-9.  The reference reached it through 500 steps
      h_g <- h_g tmp1 / tmp2 that each round h_g (not 1 - h_g) to an ulp of 1.1e-16: its value is 29 ulp, 2.0e-6 in
      log-odds (the case's ref_vs_batch), from the batch form's, which gets the log-odds directly.  When the trace's symbols
      make 1 - h_g grow again, that log-odds difference becomes visible in p.
    * k3_d3_long (N = 1e5): 1.1e-12.  lnW of a node is a log-likelihood of the size of 1e5, one ulp of which is 1.5e-11: the
      log-odds of the posterior carry 7.0e-12 of error (ref_vs_batch 2.6e-11), times h_g (1 - h_g) in p."""
    case, out, fx = orc.case_by_name(name), driven[name], load_golden(f"contexttree_{name}.npz")
    np.testing.assert_allclose(out["trace0_p"], fx["trace0_p"], rtol=1e-12, atol=0)
    assert np.array_equal(out["trace0_p"].argmax(1), fx["trace0_p"].argmax(1))
    assert np.array_equal(out["trace0_exists"], fx["trace0_exists"]) and np.array_equal(out["trace0_leaf"], fx["trace0_leaf"])
    assert np.array_equal(out["trace0_beta"], fx["trace0_beta"])
    np.testing.assert_allclose(out["trace0_g"], fx["trace0_g"], rtol=1e-12, atol=0)

    tol = 4 * float(fx["ref_vs_batch"]) + 64 * EPS
    rel = float(np.max(np.abs(out["trace_p"] - fx["trace_p"]) / fx["trace_p"]))
    err = orc.log_odds_err(out["final_g"], fx["final_g"], fx["final_exists"])
    print(f"{name} trace: relative error {rel:.3e}; final h_g log-odds error {err:.3e}, bound {tol:.3e}")
    assert np.array_equal(out["trace_p"].argmax(1), fx["trace_p"].argmax(1))
    assert np.array_equal(out["final_exists"], fx["final_exists"]) and np.array_equal(out["final_leaf"], fx["final_leaf"])
    assert np.array_equal(out["final_beta"], fx["final_beta"])
    assert err <= tol
    np.testing.assert_allclose(out["trace_p"], fx["trace_p"], rtol=TRACE_RTOL.get(name, 1e-12), atol=0)


def test_two_halves_are_not_the_whole(driven):
    """The second half starts with head samples of its own (handled as leaves above c_d_max), so two half-length updates
    differ from one full update; each matches its fixture in test_posterior_parity."""
    a, b = driven["whole"], driven["halves"]
    assert np.array_equal(a["after1_exists"], b["after2_exists"])
    assert not np.array_equal(a["after1_beta"], b["after2_beta"])     # the second half's first symbols stop above c_d_max
    ex = a["after1_exists"] != 0
    assert np.max(np.abs(a["after1_g"][ex] - b["after2_g"][ex])) > 1e-6


def test_numpy_sample_and_device_sample_agree():
    ct, rng = _ct(), np.random.default_rng(4)
    x = orc.planted_sample(3, 5000, rng)
    a = ct.LearnModel(3, 3, device="cuda:0").update_posterior(x)
    b = ct.LearnModel(3, 3, device="cuda:0").update_posterior(torch.from_numpy(x).to(torch.uint8).cuda())
    assert torch.equal(a._eng().g, b._eng().g) and torch.equal(a._eng().beta, b._eng().beta)
    assert a._engine.launch_info == "ctree_count + ctree_sweep"
