"""calc_pred_logpdf on the MI355X: the reference's fixtures, the exact recursion, tile, depth and lane-group edges, the
hash probe on tables that grew from two slots, dense against sparse bit for bit, and that nothing changes.

Bounds are ``contexttree_pred_oracle``'s, derived in its docstring; the device ``log`` stayed inside the 2 u max(1, |ln p|)
that the derivation gives a logarithm, so no measured allowance is added."""
import copy
import itertools
import pickle

import numpy as np
import pytest
import torch

import contexttree_oracle as orc
import contexttree_pred_oracle as porc
import contexttree_sparse_oracle as sorc
from conftest import load_golden

pytestmark = pytest.mark.gpu
U = porc.U


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def _model(k, D, g=0.4, hb=None, sparse=False, floor=None):
    hb = np.arange(1, k + 1) / 2.0 if hb is None else hb
    m = _ct().LearnModel(k, D, g, hb, tables="sparse" if sparse else "dense", device="cuda:0")
    if floor is not None:
        from bayesml_amd._ctsp import SparseCtreePass
        m._ctree_pass_factory = lambda k_, D_: SparseCtreePass(k_, D_, "cuda:0", floor_capacity=floor)
    return m


def _lookup(m):
    """The oracle's lookup on a host snapshot of the model's tree."""
    k, D = m.c_k, m.c_d_max
    if not m._has_root:
        return porc.no_tree
    if m._sparse:
        nd = m._eng().get_nodes()
        return porc.sparse_lookup({(int(d), int(s)): [g, b, lf] for d, s, g, b, lf in
                                   zip(nd["level"], nd["key"], nd["g"], nd["beta"], nd["leaf"])}, k, D)
    return porc.dense_lookup(m._eng().get_tables(), k, D)


def _snapshot(m):
    return m._store.save(m._eng())


def _same(a, b):
    return all(np.array_equal(a[n], b[n]) and a[n].tobytes() == b[n].tobytes() for n in a)


def _check_against(m, y, lengths, got, only=None, get=None):
    """(lnp, z, dist[, totals]) of the engine against the NumPy restatement on the model's own tree, within the bound that
    holds between two binary64 evaluations."""
    k, D = m.c_k, m.c_d_max
    lnp, z, dist = got[:3]
    rows = porc.pred_rows(y, lengths, k, D, get or _lookup(m), m.hn_g, m.hn_beta_vec, only)
    sel = np.arange(len(y)) if only is None else np.asarray(only)
    assert np.all(np.abs(dist[sel] - rows[sel]) <= porc.p_rel_reference(k, D) * rows[sel])
    want = np.log(rows[sel, np.asarray(y, dtype=np.int64)[sel]])
    assert np.all(np.abs(lnp[sel] - want) <= porc.lnp_abs_reference(k, D, want))
    clear = porc.z_clear(rows[sel], k, D)
    assert np.array_equal(z[sel][clear], rows[sel].argmax(1)[clear])
    return rows


def _check_totals(lnp, lengths, tot):
    at = np.concatenate([[0], np.cumsum(lengths)])
    for s, (a, b) in enumerate(zip(at[:-1], at[1:])):
        assert abs(tot[s] - lnp[a:b].sum()) <= max(b - a, 1) * U * np.abs(lnp[a:b]).sum()
        if a == b:
            assert tot[s] == 0.0


# ---- 1. the reference's fixtures ------------------------------------------------------------------------------------------
def _fixture_model(name, sparse):
    case = (sorc if sparse else orc).case_by_name(name)
    k, D = case["k"], case["D"]
    fx = load_golden(f"contexttree_pred_{'sparse_' if sparse else ''}{name}.npz")
    m = _model(k, D, float(fx["hn_g"]), fx["hn_beta_vec"], sparse)
    if sparse:
        lists = sorc.stage_lists(fx, "final")
        key = np.array([sorc.pack(c[:d], k, D) for d, c in zip(lists["level"], lists["ctx"])], dtype=np.int64)
        saved = dict(level=lists["level"], key=key, g=lists["g"], beta=lists["beta"], leaf=lists["leaf"])
    else:
        old = load_golden(f"contexttree_{name}.npz")
        saved = {n: old[f"final_{n}"] for n in ("g", "beta", "exists", "leaf")}
    m._store.restore(m._eng(), saved)
    m._has_root = True
    return case, fx, m


@pytest.mark.parametrize("name,sparse", [(c["name"], False) for c in orc.CASES] + [(c["name"], True) for c in sorc.CASES])
def test_reference_fixtures(name, sparse):
    case, fx, m = _fixture_model(name, sparse)
    k, D, y = case["k"], case["D"], fx["y"]
    before = _snapshot(m)
    for ref, lengths in ((fx["p_one"], None), (fx["p_split"], fx["lengths"])):
        lnp, z, dist = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True)
        assert np.all(np.abs(dist - ref) <= porc.p_rel_reference(k, D) * ref)
        want = np.log(ref[np.arange(len(y)), y])
        assert np.all(np.abs(lnp - want) <= porc.lnp_abs_reference(k, D, want))
        clear = porc.z_clear(ref, k, D)
        assert np.mean(~clear) <= 0.02
        assert np.array_equal(z[clear], ref.argmax(1)[clear])
    assert _same(before, _snapshot(m))


# ---- 2. the exact recursion -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_forced", [0.5, 1 - 2.0 ** -20, 2.0 ** -30, 0.0, 1.0])
@pytest.mark.parametrize("k,D,sparse", [(2, 4, False), (3, 3, False), (2, 4, True), (3, 3, True)])
def test_exact_oracle(k, D, sparse, g_forced):
    mp = orc._mp()
    rng = np.random.default_rng([k, D, 3])
    x = orc.planted_sample(k, 400, rng)
    m = _model(k, D, 0.3, sparse=sparse).update_posterior(x)
    eng, store = m._eng(), m._store
    ctx = [int(v) for v in x[100:102][::-1]]                  # the depth-2 node of a context the sample holds
    at = [store.address(2, store.child(1, store.child(0, 0, ctx[0]), ctx[1]))]
    g, beta, exists, leaf = eng.gather(at)
    assert exists[0]
    eng.scatter(at, [g_forced], beta, exists, leaf)
    y = np.concatenate([x[95:125], rng.integers(0, k, 30)])
    lengths = [0, 1, D, D + 1, 60 - 2 * D - 2]
    lnp, z, dist = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True)
    get = _lookup(m)
    assert get(tuple(ctx))[0] == g_forced
    start = porc.starts_of(len(y), lengths)
    assert any(i - start[i] >= 2 and [int(y[i - 1]), int(y[i - 2])] == ctx for i in range(len(y)))     # (it is visited)
    exact = porc.pred_rows_exact(y, lengths, k, D, get, m.hn_g, m.hn_beta_vec)
    for i in range(len(y)):
        for a in range(k):
            assert abs(mp.mpf(float(dist[i, a])) - exact[i][a]) <= porc.p_rel_exact(k, D) * exact[i][a]
        ln = mp.log(exact[i][int(y[i])])
        assert abs(mp.mpf(float(lnp[i])) - ln) <= float(porc.lnp_abs_exact(k, D, float(ln)))
        top = sorted(exact[i])
        if k == 1 or top[-1] - top[-2] > 2 * porc.p_rel_exact(k, D) * top[-1]:
            assert z[i] == max(range(k), key=lambda a: exact[i][a])


# ---- 3. tile and depth edges ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_models():
    k, D = 2, 5
    x = orc.planted_sample(k, 2000, np.random.default_rng(31))
    y = np.concatenate([x[300:700], np.random.default_rng(32).integers(0, k, 400)])
    return {sparse: _model(k, D, sparse=sparse).update_posterior(x) for sparse in (False, True)}, y


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("n", [1, 5, 6, 255, 256, 257, 513])
def test_sample_lengths_at_the_tile_edges(edge_models, sparse, n):
    models, y = edge_models
    m = models[sparse]
    got = m.calc_pred_logpdf(y[:n], assign=True, return_dist=True)
    assert got[0].shape == (n,) and got[1].shape == (n,) and got[2].shape == (n, 2)
    _check_against(m, y[:n], None, got)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("lengths", [
    [255, 1, 1, 0, 0, 1, 5, 6, 244, 0],          # starts on 255, 256, 257 of the first tile; two adjacent empty ones
    [0, 255, 1, 1, 5, 6, 0, 0, 245],             # the first sequence empty
    [256, 256, 1],                               # starts on the tiles' own edges
    [0, 0, 513, 0, 0],
    [1] * 300 + [213],
])
def test_sequence_starts_and_lengths(edge_models, sparse, lengths):
    models, y = edge_models
    m, y = models[sparse], y[:513]
    assert sum(lengths) == 513
    got = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True, totals=True)
    _check_against(m, y, lengths, got)
    _check_totals(got[0], lengths, got[3])
    whole = m.calc_pred_logpdf(y)
    start = porc.starts_of(513, lengths)
    deep = np.arange(513) - start >= 5                       # (positions whose context does not reach the cut)
    assert np.array_equal(got[0][deep], whole[deep])


# ---- 4. lane-group edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 128, 129, 256])
def test_lane_groups(k, sparse):
    D = 2 if k <= 65 else 1
    rng = np.random.default_rng([k, 5])
    x = rng.integers(0, k, 600)
    m = _model(k, D, sparse=sparse).update_posterior(x)
    y = np.concatenate([x[50:110], rng.integers(0, k, 60)])
    lengths = [0, 1, D, D + 1, 120 - 2 * D - 2]
    got = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True)
    _check_against(m, y, lengths, got)
    assert np.all(np.abs(got[2].sum(1) - 1) <= 2 * (k + 4 * D + 6) * U * k)
    only_z = m.calc_pred_logpdf(y, lengths=lengths, assign=True)[1]
    assert np.array_equal(only_z, got[1])


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 128, 129, 256])
def test_a_tie_gives_the_lowest_index(k, sparse):
    m = _model(k, 1, 0.4, np.full(k, 0.5), sparse)
    y = np.arange(7) % k
    lnp, z, dist = m.calc_pred_logpdf(y, assign=True, return_dist=True)        # no tree: every entry ties
    assert np.array_equal(z, np.zeros(7, np.int64)) and np.all(dist == dist[0, 0])
    beta = np.full(k, 0.5)
    beta[[k // 2, k - 1]] = 7.5                                               # the maximum twice (once at k = 1)
    m._eng().scatter([m._store.address(0, 0)], [0.0], [beta], [1], [1])
    m._has_root = True
    lnp, z, dist = m.calc_pred_logpdf(y, assign=True, return_dist=True)
    assert np.array_equal(z, np.full(7, k // 2)) and np.all(dist[:, k // 2] == dist[:, k - 1])
    assert np.all(dist.max(1) == dist[:, k // 2])


# ---- 5. the hash probe ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,D", [(2, 63), (4, 31)])
def test_sparse_probing_on_grown_tables(k, D):
    """At k = 2 every sample that holds both symbols creates both depth-1 nodes, so a path can leave the tree at depth 1
    only at k = 4, where the training sample leaves symbol 3 out."""
    from bayesml_amd import _ctpred
    rng = np.random.default_rng([k, D, 9])
    n = 3000
    x = sorc.planted_sample(k if k == 2 else 3, D, n, rng)
    m = _model(k, D, sparse=True, floor=2).update_posterior(x[:150]).update_posterior(x[150:])    # (the second one rehashes)
    eng = m._eng()
    assert eng.growths >= 1 and min(eng.caps[1:]) > 2 and eng.caps[0] == 2
    other = (int(x[D - 2]) + 1) % (2 if k == 2 else 3)
    # a run of the sample (never leaves), uniform symbols, then the sample's head behind a symbol that it does not follow
    y = np.concatenate([x[500:500 + 3 * D], rng.integers(0, k, 1000), [other], x[:D], x[1000:1000 + 3 * D],
                        rng.integers(0, k, 1000)])
    lengths = [3 * D, 1000, 0, D + 1, len(y) - 4 * D - 1001]
    i_never, i_deep = 3 * D - 1, 3 * D + 1000 + D
    only = sorted(set([0, 1, D - 1, D, i_never, i_deep, i_deep - 1, 3 * D, 3 * D + 1]
                      + list(range(3 * D + 5, 3 * D + 1000, 37)) + list(range(len(y) - 60, len(y)))))
    get = _lookup(m)
    depths = {i: porc.leave_depth(y, lengths, D, get, i) for i in only}
    # (the path of i_deep is there down to depth D - 1 and misses its last node)
    assert depths[i_never] is None and depths[i_deep] == D
    if k == 4:
        i_one = next(i for i in range(3 * D + 2, 3 * D + 1000) if y[i - 1] == 3)
        i_two = next(i for i in range(3 * D + 2, 3 * D + 1000) if y[i - 1] != 3 and y[i - 2] == 3)
        only = sorted(set(only + [i_one, i_two]))
        assert porc.leave_depth(y, lengths, D, get, i_one) == 1 and porc.leave_depth(y, lengths, D, get, i_two) == 2
    before = _snapshot(m)
    got = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True, totals=True)
    _check_against(m, y, lengths, got, only=only, get=get)
    _check_totals(got[0], lengths, got[3])
    assert m._pred_pass.upwalk == _ctpred.UP_STACK
    m._pred_pass.upwalk = _ctpred.UP_PROBE
    try:
        again = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True, totals=True)
    finally:
        m._pred_pass.upwalk = _ctpred.UP_STACK
    assert all(np.array_equal(a, b) and a.tobytes() == b.tobytes() for a, b in zip(got, again))
    assert _same(before, _snapshot(m))


# ---- 6. dense equals sparse -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,D", [(2, 10), (4, 6), (256, 2)])
def test_dense_equals_sparse(k, D):
    rng = np.random.default_rng([k, D, 11])
    x = orc.planted_sample(k, 3000, rng) if k < 256 else rng.integers(0, k, 3000) % 7 * 36
    y = np.concatenate([x[100:600], rng.integers(0, k, 500)])
    lengths = [0, 300, 1, D, D + 1, 0, 1000 - 302 - 2 * D]
    out = []
    for sparse in (False, True):
        m = _model(k, D, sparse=sparse).update_posterior(x[:2000]).update_posterior(x[2000:])
        out.append(m.calc_pred_logpdf(torch.from_numpy(y).cuda(), lengths=lengths, assign=True, return_dist=True, totals=True))
    for a, b in zip(*out):
        assert a.is_cuda and torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert np.all(np.isfinite(out[0][0].cpu().numpy())) and float(out[0][0].max()) < 0


# ---- 7. flags, determinism, totals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_flag_independence_and_totals(sparse):
    k, D = 3, 4
    rng = np.random.default_rng(12)
    x = orc.planted_sample(k, 4000, rng)
    m = _model(k, D, sparse=sparse).update_posterior(x)
    y = np.concatenate([x[:1000], rng.integers(0, k, 14003 - 1000)])
    lengths = [5000, 0, 9000, 3]                              # two sequences longer than a piece of the reduction
    assert len(y) == sum(lengths)
    base = m.calc_pred_logpdf(y, lengths=lengths)
    runs = {}
    for assign, dist, tot in itertools.product([False, True], repeat=3):
        got = m.calc_pred_logpdf(y, lengths=lengths, assign=assign, return_dist=dist, totals=tot)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == 1 + assign + dist + tot and got[0].tobytes() == base.tobytes()
        runs[(assign, dist, tot)] = got
    full, again = runs[(True, True, True)], m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True, totals=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))
    assert np.array_equal(runs[(True, False, False)][1], full[1]) and np.array_equal(runs[(False, True, False)][1], full[2])
    assert runs[(False, False, True)][1].tobytes() == full[3].tobytes()
    _check_totals(base, lengths, full[3])
    assert np.array_equal(m.calc_pred_logpdf(y), m.calc_pred_logpdf(y, lengths=[len(y)]))


# ---- 8. consistency with the product ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_it_is_the_calc_pred_dist_loop_and_reads_new_defaults(sparse):
    k, D = 3, 3
    case = orc.case_by_name("hn_changed")
    inp = orc.case_inputs(case)
    m = _model(k, D, case["h0_g"], sparse=sparse).update_posterior(inp["x1"])
    y = np.concatenate([inp["x1"][40:55], np.random.default_rng(13).integers(0, k, 25)])
    lengths = [0, 1, 3, 4, 32]
    at = np.concatenate([[0], np.cumsum(lengths)])

    def loop_rows():
        loop = copy.deepcopy(m)
        rows = np.zeros((len(y), k))
        for a, b in zip(at[:-1], at[1:]):
            for i in range(a, b):
                rows[i] = loop.calc_pred_dist(y[a:i + 1]).p_theta_vec
        return rows

    def compare():
        lnp, z, dist = m.calc_pred_logpdf(y, lengths=lengths, assign=True, return_dist=True)
        rows = loop_rows()
        assert np.all(np.abs(dist - rows) <= porc.p_rel_reference(k, D) * rows)
        want = np.log(rows[np.arange(len(y)), y])
        assert np.all(np.abs(lnp - want) <= porc.lnp_abs_reference(k, D, want))
        clear = porc.z_clear(rows, k, D)
        assert np.array_equal(z[clear], rows.argmax(1)[clear])
        return lnp
    first = compare()
    get = _lookup(m)
    left = np.array([porc.leave_depth(y, lengths, D, get, i) is not None for i in range(len(y))])
    assert left.any() and not left.all()
    # new defaults, as the hn_changed case sets them: fill_existing gives them to every existing node too, so the tree is
    # put back and only the positions that leave it may move
    saved = _snapshot(m)
    m.set_hn_params(hn_g=case["hn2"][0], hn_beta_vec=np.array(case["hn2"][1]))
    m._store.restore(m._eng(), saved)
    second = compare()
    assert np.array_equal(first[~left], second[~left]) and not np.array_equal(first[left], second[left])


# ---- 9. nothing changes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("value,dtype,text", [(255, np.uint8, "x.max() must smaller than c_k:3"), (3, np.int64, "x.max() must smaller than c_k:3"),
                                              (-1, np.int64, None), (-7, np.int32, None)])
def test_a_refused_sample_changes_nothing(sparse, where, value, dtype, text):
    from bayesml_amd import _check
    from bayesml_amd._exceptions import DataFormatError
    k, D = 3, 3
    x = orc.planted_sample(k, 500, np.random.default_rng(14))
    m = _model(k, D, sparse=sparse).update_posterior(x)
    before, blob, p_before = _snapshot(m), pickle.dumps(m), m.p_theta_vec.copy()
    y = x[:300].astype(dtype)
    y[{"first": 0, "middle": 256, "last": 299}[where]] = value
    for kw in (dict(), dict(assign=True, return_dist=True, lengths=[100, 200], totals=True)):
        with pytest.raises(DataFormatError) as info:
            m.calc_pred_logpdf(y, **kw)
        assert str(getattr(info.value, "value", info.value)) == (text or "x" + _check.SAMPLE_MSG["nonneg_ints"])
    assert _same(before, _snapshot(m)) and pickle.dumps(m) == blob and np.array_equal(p_before, m.p_theta_vec)
    good = m.calc_pred_logpdf(x[:300])
    assert np.all(np.isfinite(good)) and _same(before, _snapshot(m)) and pickle.dumps(m) == blob


@pytest.mark.parametrize("sparse", [False, True])
def test_a_model_without_a_tree(sparse):
    m = _model(3, 3, sparse=sparse)
    y = np.array([2, 0, 1, 1, 2, 0, 0])
    lnp, z, dist, tot = m.calc_pred_logpdf(y, lengths=[3, 0, 4], assign=True, return_dist=True, totals=True)
    want = m.hn_beta_vec / m.hn_beta_vec.sum()
    assert np.all(np.abs(dist - want) <= 4 * U * want) and np.array_equal(z, np.full(7, 2)) and m.hn_root is None
    assert np.all(np.abs(lnp - np.log(want[y])) <= 4 * U * np.maximum(1, np.abs(lnp)))
    _check_totals(lnp, [3, 0, 4], tot)


# ---- 10. inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_dtypes_and_views(sparse):
    k, D, n = 3, 4, 700
    rng = np.random.default_rng(15)
    x = orc.planted_sample(k, 2000, rng)
    m = _model(k, D, sparse=sparse).update_posterior(x)
    big = np.concatenate([x[:400], rng.integers(0, k, n + 3 - 400)])
    want = {s: m.calc_pred_logpdf(big[s:s + n], lengths=[n - 300, 300], assign=True) for s in range(4)}
    for dt in (torch.uint8, torch.int32, torch.int64):
        buf = torch.from_numpy(big).to(dt).cuda()
        for s in range(4):
            lnp, z = m.calc_pred_logpdf(buf[s:s + n], lengths=[n - 300, 300], assign=True)
            assert isinstance(lnp, torch.Tensor) and lnp.is_cuda and lnp.dtype == torch.float64 and lnp.shape == (n,)
            assert z.is_cuda and z.dtype == torch.int64
            assert np.array_equal(lnp.cpu().numpy(), want[s][0]) and np.array_equal(z.cpu().numpy(), want[s][1])
        strided = torch.from_numpy(np.repeat(big, 2)).to(dt).cuda()[::2]
        assert np.array_equal(m.calc_pred_logpdf(strided[:n], lengths=[n - 300, 300]).cpu().numpy(), want[0][0])
    for dt in (np.uint8, np.int32, np.int64):
        got = m.calc_pred_logpdf(big[:n].astype(dt), lengths=torch.tensor([n - 300, 300]), assign=True)
        assert isinstance(got[0], np.ndarray) and np.array_equal(got[0], want[0][0]) and np.array_equal(got[1], want[0][1])
    assert m.calc_pred_logpdf(int(big[0]))[0] == want[0][0][0]
