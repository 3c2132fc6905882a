"""contexttree with tables="sparse" on the MI355X: the ctsp_* kernels against the dense engine where both run, against the
reference's fixtures beyond the dense limit, and the mechanics of the hash tables."""
import copy
import functools
import pickle
import warnings

import numpy as np
import pytest
import torch

import contexttree_oracle as orc
import contexttree_sparse_oracle as sorc
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NAMES = [c["name"] for c in sorc.CASES]
TORCH_DT = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
BOTH = ((2, 3), (3, 4), (4, 6), (2, 12), (5, 1))


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _sparse(k, D, **kw):
    from bayesml_amd import _ctsp
    return _ctsp.SparseCtreePass(k, D, torch.device("cuda", 0), **kw)


def _dense(k, D):
    from bayesml_amd import _ctree
    return _ctree.CtreePass(k, D, torch.device("cuda", 0))


def _model(k, D, *a):
    return _ct().LearnModel(k, D, *a, tables="sparse", device="cuda:0")


def _skewed(k, n, rng):
    return rng.choice(k, n, p=rng.dirichlet(np.ones(k) * 0.3))


def _dense_lists(t, k, D, extra=None):
    """Canonical lists of dense tables (and of ``extra``, a per-index array such as map_leaf)."""
    off = orc.offsets(k, D)
    rows = []
    for i in np.flatnonzero(t["exists"]):
        d = int(np.searchsorted(off, i, side="right") - 1)
        s = int(i - off[d])
        ctx = [(s // k ** j) % k for j in range(d)]
        rows.append((d, sorc.pack(ctx, k, D), ctx, i))
    rows.sort(key=lambda r: (r[0], r[1]))
    idx = np.array([r[3] for r in rows], dtype=np.int64)
    ctx = np.zeros((len(rows), D), dtype=np.uint8)
    for r, row in enumerate(rows):
        ctx[r, :row[0]] = row[2]
    out = dict(level=np.array([r[0] for r in rows], dtype=np.int32), ctx=ctx, g=t["g"][idx], beta=t["beta"][idx],
               leaf=t["leaf"][idx])
    return (out, extra[idx]) if extra is not None else out


def _bitwise_equal(a, b):
    return (sorc.same_node_set(a, b) and np.array_equal(a["beta"], b["beta"]) and np.array_equal(a["leaf"], b["leaf"])
            and np.array_equal(a["g"].view(np.int64), b["g"].view(np.int64)))


def _samples(k, rng):
    """name -> list of updates: the oracle cases' planted source, a skewed one, an all-equal one, a two-update sequence."""
    return {"planted": [orc.planted_sample(k, 3000, rng)], "skewed": [_skewed(k, 3001, rng)],
            "all_equal": [np.full(2049, k - 1)], "two_updates": [orc.planted_sample(k, 1500, rng), _skewed(k, 700, rng)],
            "short": [rng.integers(0, k, 2)]}


# ---- same answers as the dense engine -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,D", BOTH)
def test_bitwise_equal_to_the_dense_engine(k, D):
    """Node set, leaf, h_beta_vec AND h_g bit for bit, and map_leaf of every existing node, on the same input."""
    rng = np.random.default_rng(100 * k + D)
    hb = np.arange(1, k + 1) / 2.0
    for name, updates in _samples(k, rng).items():
        sp, de = _sparse(k, D), _dense(k, D)
        for j, x in enumerate(updates):
            xd = torch.from_numpy(np.asarray(x)).to(torch.uint8).cuda()
            assert sp.update(xd, 0.4, hb) == de.update(xd, 0.4, hb) == (len(x), 0)
            want, want_ml = _dense_lists(de.get_tables(), k, D, de.map_leaf(0.4))
            got = sorc.engine_lists(sp.get_nodes(), k, D)
            assert _bitwise_equal(got, want), (name, j)
            assert np.array_equal(sp.map_leaf(0.4), want_ml), (name, j)
        assert sp.launch_info == "ctsp_map"


@pytest.mark.parametrize("k,D", BOTH)
def test_estimate_params_equal_to_the_dense_model(k, D):
    ct, rng = _ct(), np.random.default_rng(k + D)
    x = orc.planted_sample(k, 2000, rng)
    trees = []
    for tables in ("dense", "sparse"):
        m = ct.LearnModel(k, D, 0.6, np.arange(1, k + 1) / 2.0 + 1, tables=tables, device="cuda:0").update_posterior(x)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            trees.append(sorc.map_tree_to_lists(m.estimate_params(visualize=False), k, D))
    a, b = trees
    assert sorc.same_node_set(a, b) and np.array_equal(a["leaf"], b["leaf"]) and np.array_equal(a["g"], b["g"])
    assert np.array_equal(a["theta"], b["theta"], equal_nan=True)


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driven():
    """Every sparse fixture case walked through the drop-in on the GPU, once."""
    ct = _ct()
    make = functools.partial(ct.LearnModel, tables="sparse", device="cuda:0")
    return {case["name"]: sorc.drive(ct, case, sorc.case_inputs(case), make=make)[0] for case in sorc.CASES}


@pytest.mark.parametrize("name", NAMES)
def test_posterior_parity(name, driven):
    """Node set, leaf and h_beta_vec exactly; h_g in log-odds to 4 x ref_vs_batch + 64 eps of the case."""
    out, fx = driven[name], load_golden(f"contexttree_sparse_{name}.npz")
    tol = 4 * float(fx["ref_vs_batch"]) + 64 * EPS
    for stage in ("prior", "after1", "after2"):
        if f"{stage}_level" not in fx:
            assert f"{stage}_level" not in out
            continue
        got, ref = sorc.stage_lists(out, stage), sorc.stage_lists(fx, stage)
        assert sorc.same_node_set(got, ref)
        assert np.array_equal(got["beta"], ref["beta"]) and np.array_equal(got["leaf"], ref["leaf"])
        err = sorc.g_err(got, ref)
        print(f"{name} {stage}: {len(ref['g'])} nodes, log-odds error {err:.3e}, bound {tol:.3e}")
        assert err <= tol


@pytest.mark.parametrize("name", NAMES)
def test_pred_dist_and_trace(name, driven):
    """calc_pred_dist on three contexts (the second leaves the tree) and the 50-step pred_and_update trace.  p is a
    mixture along one path, so |dp| <= sum over the path of |dg| <= (D + 1) tol / 4 with tol the posterior's log-odds
    bound (tests/test_contexttree.py derives the same from ref_vs_batch); the trace by ``trace_p_atol``."""
    case, out, fx = sorc.case_by_name(name), driven[name], load_golden(f"contexttree_sparse_{name}.npz")
    tol = 4 * float(fx["ref_vs_batch"]) + 64 * EPS
    for j in range(3):
        print(f"{name} pred{j}: max |dp| {np.max(np.abs(out[f'pred{j}'] - fx[f'pred{j}'])):.3e}")
        np.testing.assert_allclose(out[f"pred{j}"], fx[f"pred{j}"], rtol=1e-12, atol=(case["D"] + 1) * tol / 4)
        assert out[f"pred{j}_argmax"] == fx[f"pred{j}_argmax"]
        assert int(out[f"pred{j}_nodes"]) == int(fx[f"pred{j}_nodes"])
    print(f"{name} trace: max |dp| {np.max(np.abs(out['trace_p'] - fx['trace_p'])):.3e}")
    np.testing.assert_allclose(out["trace_p"], fx["trace_p"], rtol=0, atol=orc.trace_p_atol(tol, case["D"]))
    assert np.array_equal(out["trace_p"].argmax(1), fx["trace_p"].argmax(1))
    assert int(out["final_nodes"]) == int(fx["final_nodes"])


@pytest.mark.parametrize("name", [c["name"] for c in sorc.CASES if c["map_stored"]])
def test_map_tree(name, driven):
    out, fx = driven[name], load_golden(f"contexttree_sparse_{name}.npz")
    tol = 4 * float(fx["ref_vs_batch"]) + 64 * EPS
    got, ref = ({n: t[f"map_{n}"] for n in ("level", "ctx", "leaf", "g", "theta")} for t in (out, fx))
    assert sorc.same_node_set(got, ref) and np.array_equal(got["leaf"], ref["leaf"])
    assert sorc.g_err(got, ref) <= tol
    assert np.array_equal(np.isnan(got["theta"]), np.isnan(ref["theta"]))
    np.testing.assert_allclose(np.nan_to_num(got["theta"]), np.nan_to_num(ref["theta"]), rtol=1e-12, atol=0)


def test_map_tree_too_large_is_refused():
    """(16, 6) at hn_g = 1: every missing node is the root of a full subtree; the count stops it before a node is built."""
    from bayesml_amd._engine import EngineLimitError
    m = _model(16, 6, 1.0)
    m.update_posterior(np.random.default_rng(1).integers(0, 16, 300))
    with pytest.raises(EngineLimitError, match="MAP tree"):
        m.estimate_params(visualize=False)


# ---- table mechanics ------------------------------------------------------------------------------------------------------------
def test_growth_and_memory_budget():
    """The (4, 12) two-update case from a floor capacity of 2: every level grows by rehash and the results do not change; a
    budget of a few kilobytes refuses the update and leaves the posterior bit-identical."""
    from bayesml_amd._engine import EngineLimitError
    case = sorc.case_by_name("k4_d12")
    inp, hb = sorc.case_inputs(case), np.arange(1, 5) / 2.0
    tiny, roomy = _sparse(4, 12, floor_capacity=2), _sparse(4, 12)
    assert tiny.caps == [2] * 13
    for x in (inp["x1"], inp["x2"]):
        xd = torch.from_numpy(x).cuda()
        assert tiny.update(xd, 0.5, hb) == roomy.update(xd, 0.5, hb) == (len(x), 0)
        assert _bitwise_equal(sorc.engine_lists(tiny.get_nodes(), 4, 12), sorc.engine_lists(roomy.get_nodes(), 4, 12))
    assert tiny.growths >= 1 and tiny.caps[12] == 8192 and roomy.caps[0] == 64 and all(c & (c - 1) == 0 for c in tiny.caps)
    used = [int(v) for v in np.bincount(tiny.get_nodes()["level"], minlength=13)]
    assert all(2 * u <= c for u, c in zip(used, tiny.caps))
    before = tiny.get_nodes()
    tiny.budget_bytes = 4096
    with pytest.raises(EngineLimitError, match="memory budget of 4096 bytes"):
        tiny.update(torch.from_numpy(np.tile(inp["x1"], 4)).cuda(), 0.5, hb)      # (6000 samples: level 12 must grow)
    with pytest.raises(EngineLimitError):
        _sparse(4, 12, budget_bytes=1024, floor_capacity=2)
    after = tiny.get_nodes()
    assert all(np.array_equal(before[n], after[n]) for n in before)
    assert before["g"].tobytes() == after["g"].tobytes()


def test_find_gather_scatter():
    from bayesml_amd import _ctsp
    k, D = 3, 20
    eng = _sparse(k, D, floor_capacity=2)
    ctx = [2, 0, 1, 1, 2]
    path = [(d, _ctsp.key_of(ctx[:d], k, D)) for d in range(len(ctx) + 1)]
    assert np.all(eng.find([p[0] for p in path], [p[1] for p in path]).cpu().numpy() == -1)
    g, beta = np.linspace(0.1, 0.6, 6), np.arange(18.0).reshape(6, 3) + 0.5
    eng.scatter(path, g, beta, np.ones(6, np.uint8), np.zeros(6, np.uint8))
    slots = eng.find([p[0] for p in path], [p[1] for p in path]).cpu().numpy()
    assert np.all(slots >= 0) and len(set(slots)) == 6
    assert all(eng.off[d] <= s < eng.off[d + 1] for (d, _), s in zip(path, slots))
    got = eng.gather(path + [(6, _ctsp.key_of(ctx + [0], k, D))])
    assert np.array_equal(got[0][:6], g) and np.array_equal(got[1][:6], beta) and list(got[2]) == [1] * 6 + [0]
    # a key with bits outside its level, and a level outside 0..D, are absent
    assert list(eng.find([1, D + 1, -1], [path[3][1], 0, 0]).cpu().numpy()) == [-1, -1, -1]
    nodes = eng.get_nodes()
    assert list(nodes["level"]) == list(range(6)) and [int(v) for v in nodes["key"]] == [p[1] for p in path]


# ---- keys at the edge -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,D", [(2, 63), (4, 31), (256, 7)])
def test_widest_keys(k, D):
    """Samples of the largest symbol only (every key bit in use) and of 0 only (every key is 0: levels differ by table
    alone), N on both sides of D.  Node set, h_beta_vec and leaf equal the sparse oracle's.  h_g: with the prior 1/2 per
    symbol and N <= D + 5 <= 68 every lgamma the oracle takes is below lnG(68 + 128) < 600, scipy's gammaln is good to a
    few ulp of that, a node takes four of them and a path has D + 1 nodes: 16 x 600 eps (D + 1) in log-odds."""
    hb = np.ones(k) / 2
    tol = 16 * 600 * EPS * (D + 1)
    for sym in (k - 1, 0):
        for n in (D - 1, D, D + 1, D + 5):
            x = np.full(n, sym)
            eng = _sparse(k, D)
            assert eng.update(torch.from_numpy(x).to(torch.uint8).cuda(), 0.5, hb) == (n, 0)
            got = sorc.engine_lists(eng.get_nodes(), k, D)
            want = sorc.nodes_to_lists(sorc.batch_update(x, k, D, {}, 0.5, hb), k, D)
            assert sorc.same_node_set(got, want), (sym, n)
            assert len(want["level"]) == min(n, D + 1)
            assert np.array_equal(got["beta"], want["beta"]) and np.array_equal(got["leaf"], want["leaf"])
            assert sorc.g_err(got, want) <= tol, (sym, n)
            if sym == k - 1 and n > D:
                assert int(eng.get_nodes()["key"][-1]) == 2 ** (sorc.bits(k) * D) - 1


# ---- bad symbols ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bad_value", [("i32", -1), ("i64", -1), ("u8", 4), ("i32", 4), ("i64", 4), ("u8", 255),
                                             ("i32", 255), ("i64", 255)])
def test_bad_symbols(dtype, bad_value):
    ct = _ct()
    k, D, n = 4, 12, 5000
    rng = np.random.default_rng(3)
    clean = rng.integers(0, k, n)
    m = _model(k, D)
    m.update_posterior(clean[:500])
    before = m._eng().get_nodes()
    msg = ("x must be int or a numpy.ndarray whose dtype is int. Its values must be non-negative (including 0)."
           if bad_value < 0 else f"x.max() must smaller than c_k:{k}")
    for place in (0, 5, n // 2, n - 1):          # in the head, in the middle, in the last position
        x = clean.copy()
        x[place] = bad_value
        with pytest.raises(ct._contexttree.DataFormatError) as err:
            m.update_posterior(torch.from_numpy(x).to(TORCH_DT[dtype]).cuda())
        assert err.value.value == msg
        after = m._eng().get_nodes()
        assert all(a.tobytes() == after[name].tobytes() for name, a in before.items()), place
    # and the model still learns afterwards, as if the refused samples had never been seen
    fresh = _model(k, D).update_posterior(clean[:500]).update_posterior(clean[500:900])
    m.update_posterior(clean[500:900])
    a, b = m._eng().get_nodes(), fresh._eng().get_nodes()
    assert all(a[name].tobytes() == b[name].tobytes() for name in a)


# ---- other properties -------------------------------------------------------------------------------------------------------------
def test_untouched_nodes_keep_their_bits():
    k, D = 4, 12
    rng = np.random.default_rng(5)
    first, second = rng.integers(0, k, 800), rng.integers(0, k, 300)
    eng = _sparse(k, D)
    hb = np.array([1.0, 2.0, 3.0, 0.5])
    eng.update(torch.from_numpy(first).cuda(), 0.4, hb)
    before = eng.get_nodes()
    eng.update(torch.from_numpy(second).cuda(), 0.4, hb)
    after = eng.get_nodes()
    touched = set()
    for d in range(D + 1):
        touched |= {(d, int(s)) for s in sorc.level_keys(second, k, D, d)}
    pos = {(int(d), int(s)): i for i, (d, s) in enumerate(zip(after["level"], after["key"]))}
    kept = [(i, pos[(int(d), int(s))]) for i, (d, s) in enumerate(zip(before["level"], before["key"]))
            if (int(d), int(s)) not in touched]
    assert len(kept) > 1000
    i, j = (np.array(v) for v in zip(*kept))
    for name in ("g", "beta", "leaf"):
        assert before[name][i].tobytes() == after[name][j].tobytes(), name


def test_two_runs_and_pickle():
    rng = np.random.default_rng(9)
    x, x2 = _skewed(4, 20000, rng), rng.integers(0, 4, 500)
    a, b = _model(4, 12).update_posterior(x), _model(4, 12).update_posterior(torch.from_numpy(x).to(torch.uint8).cuda())
    na, nb = a._eng().get_nodes(), b._eng().get_nodes()
    assert all(na[name].tobytes() == nb[name].tobytes() for name in na)
    assert a._engine.launch_info == "ctsp_count + ctsp_levelup + ctsp_sweep"
    c = pickle.loads(pickle.dumps(a))
    assert c._engine is None and c._sparse
    assert _bitwise_equal(sorc.tree_to_lists(c.hn_root, 4, 12), sorc.tree_to_lists(a.hn_root, 4, 12))
    a.update_posterior(x2)
    c.update_posterior(x2)
    assert _bitwise_equal(sorc.engine_lists(a._eng().get_nodes(), 4, 12), sorc.engine_lists(c._eng().get_nodes(), 4, 12))
    d = copy.deepcopy(a)
    assert np.array_equal(d.calc_pred_dist(x2[:20]).p_theta_vec, a.calc_pred_dist(x2[:20]).p_theta_vec)


def test_setters_on_sparse_storage(tmp_path):
    ct = _ct()
    k, D = 4, 12
    gen = ct.GenModel(k, D, h_g=0.3, seed=sorc.H0_ROOT_SEED).gen_params()
    m = _model(k, D, 0.4, np.array([1.0, 2.0, 3.0, 4.0]), gen.root)
    t1 = sorc.tree_to_lists(m.hn_root, k, D)
    assert len(t1["level"]) > 900 and 0 < t1["leaf"][t1["level"] < D].sum() < (t1["level"] < D).sum()
    m2 = _model(k, D, 0.4, np.array([1.0, 2.0, 3.0, 4.0]))
    assert m2.hn_root is None
    m2.set_hn_params(hn_root=m.hn_root)           # materialise -> scatter -> materialise
    assert _bitwise_equal(t1, sorc.tree_to_lists(m2.hn_root, k, D))
    m2.set_hn_params(hn_g=0.25, hn_beta_vec=np.array([2.0, 2.0, 5.0, 1.0]))
    t3 = sorc.tree_to_lists(m2.hn_root, k, D)
    assert np.all(t3["g"][t3["level"] < D] == 0.25) and np.all(t3["g"][t3["level"] == D] == 0.0)
    assert np.all(t3["beta"] == np.array([2.0, 2.0, 5.0, 1.0]))
    m.update_posterior(np.random.default_rng(2).integers(0, k, 400))
    m.overwrite_h0_params()                       # h0 <- hn, then hn <- h0: the posterior keeps h0's nodes
    t4, t5 = sorc.tree_to_nodes(m.h0_root, k, D), sorc.tree_to_nodes(m.hn_root, k, D)
    assert set(t4) <= set(t5) and all(t4[i][0] == t5[i][0] and np.array_equal(t4[i][1], t5[i][1]) for i in t4)
    # save / load: a tree without leaf flags above the maximal depth comes back whole (superposition stops at a leaf,
    # ref:547-576); on top, the superposition gives every inner node all its children, with the defaults
    m4 = _model(k, D).update_posterior(np.random.default_rng(3).integers(0, k, 400))
    m4.save_hn_params(str(tmp_path / "hn.pkl"))
    m3 = _model(k, D).load_hn_params(str(tmp_path / "hn.pkl"))
    t7, t8 = sorc.tree_to_nodes(m4.hn_root, k, D), sorc.tree_to_nodes(m3.hn_root, k, D)
    assert set(t7) <= set(t8) and all(np.all(t8[i][1] == 0.5) and t8[i][0] in (0.0, 0.5) for i in set(t8) - set(t7))
    assert all(t7[i][0] == t8[i][0] and np.array_equal(t7[i][1], t8[i][1]) and t7[i][2] == t8[i][2] for i in t7)
    m.reset_hn_params()
    t6 = sorc.tree_to_nodes(m.hn_root, k, D)
    assert set(t6) >= set(t4) and all(t4[i][0] == t6[i][0] and np.array_equal(t4[i][1], t6[i][1]) for i in t4)
    one = _model(k, D).update_posterior(np.array([3]))           # N = 1
    assert list(sorc.tree_to_nodes(one.hn_root, k, D)) == [(0, 0)] and one.make_prediction(loss="0-1") in range(k)


def test_count_with_a_hot_key_across_workgroup_ranges():
    """N = 3e5 (74 workgroup ranges of 4096): one symbol nine times in ten, so one key takes most adds from every range;
    the deepest level's counts against NumPy."""
    k, D, n = 4, 12, 300000
    rng = np.random.default_rng(12)
    x = np.where(rng.random(n) < 0.9, 2, rng.integers(0, k, n))
    eng = _sparse(k, D)
    xd = torch.from_numpy(x).to(torch.uint8).cuda()
    eng._reserve(n)
    eng.count(xd)
    assert [int(v) for v in eng._status.cpu()] == [n, 0, 0, 0]
    keys = sorc.level_keys(x, k, D, D)
    uniq, inv = np.unique(keys, return_inverse=True)
    want = np.zeros((len(uniq), k), dtype=np.int64)
    np.add.at(want, (inv, x[D:]), 1)
    slots = eng.find([D] * len(uniq), uniq)
    assert bool((slots >= 0).all())
    assert np.array_equal(eng._cnt[slots].cpu().numpy(), want) and int(eng._cnt.sum()) == n - D
    assert int((eng.key[eng.off[D]:] != -1).sum()) == len(uniq) and want.max() > n // 4
