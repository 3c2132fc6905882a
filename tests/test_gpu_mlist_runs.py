"""The persistent form of the list M-step (bayesml_amd/csrc/mstep.h, "runs"): the components' lists, each padded to whole
batches of 64 entries and laid end to end, are cut into G runs of equal batch counts; a run writes one slab per component it
meets (slab g + k), reduce_chunks_kernel adds the slabs of the runs that met a component in ascending run order.
GMMVB_MLIST_RUNS=<n> (a developer switch: behind GMMVB_DEBUG, read when the workspace is created) caps G at n, so that small
lists put several components into one run and several runs into one component.

Run edges.  One forced pruned E-step over far-apart clusters of chosen sizes with the parameters at their means leaves
component k the list of cluster k's rows with responsibilities that are exactly 1 (every other component's share underflows),
and an empty list to a component without a cluster.  The statistics block of the list M-step that follows is compared,
entry by entry, with sums in numpy.longdouble over the responsibilities the workspace reads out and the same rows.

The bound.  An entry is a sum of n terms t_j = r_j x'_a x'_b (B), r_j x'_a (a) or r_j (ns), x' = x - pivot, n the length of
the component's list.  With u = 2^-53: x' is one rounded subtraction per factor (relative u each; the f32 row itself is exact
in f64), the M-step's own r = exp(ln rho - lse) and the read-out's may differ in the last place (2 u), r x'_a is one rounded
product (u) and the MFMA's multiply-add one more (u): a term as the kernel forms it is within 6 u |t_j| of the exact one - 8 u
with the slack of the second-order terms.  Adding n such terms in any order of f64 additions - along a run, then over the
run slabs - adds at most (n - 1) u times the sum of their absolute values (each partial sum is bounded by it).  Together
|delta| <= (n + 7) u sum|t_j| <= (n + 8) 2^-52 sum|t_j|, whatever G is and wherever the runs are cut; the same holds for the
chunk form.  h = sum r ln r is 0 exactly (r is 0 or 1) and B comes out exactly symmetric (one triangle is computed, the other
is its copy).

Delta lists.  A forced pruned fit settles rows; the rows that settle or come loose go through the same kernels as signed
delta lists (weights +-1) into the cache of settled rows.  The fit's posterior under 1, 3 and the device's own number of
runs, without the cache, and through the dense M-step must agree within what tests/test_gpu_sparse_parity.py grants a sparse
variant against its reference posterior: 1e-6 relative (1e-5 for the scatter matrices).

Every case without the switch also passes against the library of the commit before the runs (profiles/mlist_runs.md): the
bounds are the sums' own, not the new code's."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

LD = np.longdouble
KEYS = ("GMMVB_ESTEP_PRUNE", "GMMVB_MSTEP_SPARSE", "GMMVB_MSTEP_CACHE", "GMMVB_DEBUG", "GMMVB_MLIST_RUNS")
RUNS = (1, 2, 3, 7, None)


def dev():
    return torch.device("cuda", 0)


class env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KEYS}
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def switches(runs, **more):
    kv = {"GMMVB_ESTEP_PRUNE": "force", **more}
    if runs is not None:
        kv.update(GMMVB_DEBUG="1", GMMVB_MLIST_RUNS=str(runs))
    return kv


# ---- run edges -------------------------------------------------------------------------------------------------------------
SHAPES = {"d128-f32": (128, np.float32, "mstep_list_f64<T=8,x=f32>"), "d64-f32": (64, np.float32, "mstep_list_f64<T=4,x=f32>"),
          "d40-f64": (40, np.float64, "mstep_list_f64<T=3,centred-f64>")}
LENGTHS = {"ragged": [0, 5, 64, 65, 0, 4096, 1], "one-of-three": [8000, 0, 0], "whole-batches": [64 * 33, 0],
           "one-over": [64 * 33 + 1, 0]}


def clusters(D, lengths, dtype, seed):
    rng = np.random.default_rng(seed)
    K = len(lengths)
    mu = 8.0 * rng.standard_normal((K, D))
    z = rng.permutation(np.repeat(np.arange(K), lengths))
    return (mu[z] + rng.standard_normal((len(z), D))).astype(dtype), mu, z


def list_pass(x, mu, kv):
    """One E-step and list M-step of a fresh workspace: statistics block, responsibilities, pivot, launch line."""
    from bayesml_amd import _kside
    from bayesml_amd._engine import DataPass
    N, D = x.shape
    K = mu.shape[0]
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev())   # noqa: E731
    qd = _kside.features(_kside.PostT(t(np.full(K, N / K)), t(mu), t(np.full(K, 100.0)), t(np.full(K, D + 100.0)),
                                      t(np.tile((D + 100.0) * np.eye(D), (K, 1, 1)))))
    xd = torch.from_numpy(x).to(dev())
    with env(kv):
        eng = DataPass(K, D, xd.dtype, N, dev())
    eng.set_pivot(xd[:4096].to(torch.float64).mean(dim=0))
    eng.prepare_rows(xd)
    eng.set_params(qd.c, qd.m, qd.u)
    stats = eng.estep_mstep(xd).clone()
    info, lists = eng.launch_info, eng.pass_counts()["mstep_list"]
    r = eng.responsibilities().cpu().numpy()
    pivot = eng.pivot.cpu().numpy()
    parts = [p.cpu().numpy() for p in eng.split_stats(stats)]
    eng.close()
    return stats, parts, r, pivot, info, lists


def host_sums(x, r, pivot):
    """Per component: the sums and the sums of the addends' absolute values, in longdouble, and the list lengths."""
    K, D = r.shape[1], x.shape[1]
    xq = x.astype(LD) - pivot.astype(LD)
    ns, a, B = np.zeros(K, LD), np.zeros((K, D), LD), np.zeros((K, D, D), LD)
    a_abs, B_abs, n = np.zeros((K, D), LD), np.zeros((K, D, D), LD), np.zeros(K, np.int64)
    for k in range(K):
        rows = np.nonzero(r[:, k] > 0)[0]
        n[k] = len(rows)
        if not len(rows):
            continue
        w, xs = r[rows, k].astype(LD), xq[rows]
        wx = w[:, None] * xs
        ns[k], a[k], a_abs[k] = w.sum(), wx.sum(axis=0), np.abs(wx).sum(axis=0)
        B[k], B_abs[k] = wx.T @ xs, np.abs(wx).T @ np.abs(xs)
    return dict(ns=ns, a=a, B=B, a_abs=a_abs, B_abs=B_abs, n=n)


_cases = {}


def lengths_of(shape, lengths):
    """The case's list lengths.  f64 rows at three feature tiles have no pruned E-step: their lists follow a dense E-step
    that counted its active pairs, which the library does from N K = 2^18 on - one more cluster brings the rows up to that."""
    want = list(LENGTHS[lengths])
    if SHAPES[shape][1] is np.float64:
        want.append(max(0, -(-2 ** 18 // (len(want) + 1)) - sum(want)))
    return want


def run_edge_case(shape, lengths):
    """The case's rows, its statistics under every number of runs (one workspace each), and the host sums - made once."""
    key = (shape, lengths)
    if key not in _cases:
        D, dtype, kernel = SHAPES[shape]
        x, mu, z = clusters(D, lengths_of(shape, lengths), dtype, 7 * D + len(LENGTHS[lengths]))
        got = {runs: list_pass(x, mu, switches(runs)) for runs in RUNS}
        r = got[None][2]
        for runs in RUNS:                                  # the same E-step every time: the same responsibilities
            assert np.array_equal(got[runs][2], r)
        _cases[key] = (x, z, got, host_sums(x, r, got[None][3]), kernel)
    return _cases[key]


@pytest.mark.parametrize("lengths", sorted(LENGTHS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_statistics_within_the_derived_bound(shape, lengths):
    x, z, got, ref, kernel = run_edge_case(shape, lengths)
    want = np.array(lengths_of(shape, lengths))
    r = got[None][2]
    assert np.array_equal(np.unique(r), [0.0, 1.0]) and np.array_equal(r[np.arange(len(z)), z], np.ones(len(z)))
    assert np.array_equal(ref["n"], want)
    for runs in RUNS:
        _stats, (ns, h, a, B), _r, _p, info, lists = got[runs]
        assert kernel in info and lists == 1, info
        eps = (ref["n"] + 8).astype(LD) * LD(2.0) ** -52
        d_ns = np.abs(ns.astype(LD) - ref["ns"])
        d_a = np.abs(a.astype(LD) - ref["a"])
        d_B = np.abs(B.astype(LD) - ref["B"])
        worst = [float(np.max(d / np.maximum(lim, LD(1e-300))))
                 for d, lim in ((d_ns, eps * ref["ns"]), (d_a, eps[:, None] * ref["a_abs"]), (d_B, eps[:, None, None] * ref["B_abs"]))]
        print("mlist-runs", shape, lengths, "runs", runs, "largest error / bound (ns, a, B):", worst)
        assert np.array_equal(ns, want.astype(np.float64))            # (sums of ones)
        assert np.all(h == 0.0)
        assert np.all(d_a <= eps[:, None] * ref["a_abs"])
        assert np.all(d_B <= eps[:, None, None] * ref["B_abs"])
        assert np.array_equal(B, np.swapaxes(B, 1, 2))
        empty = want == 0
        assert np.all(a[empty] == 0.0) and np.all(B[empty] == 0.0)


@pytest.mark.parametrize("runs", [3, None])
def test_two_runs_of_a_case_give_the_same_bits(runs):
    x, z, got, _ref, _kernel = run_edge_case("d128-f32", "ragged")
    D, dtype, _ = SHAPES["d128-f32"]
    _x, mu, _z = clusters(D, LENGTHS["ragged"], dtype, 7 * D + len(LENGTHS["ragged"]))
    again = list_pass(x, mu, switches(runs))[0]
    assert torch.equal(again, got[runs][0])


# ---- delta lists -----------------------------------------------------------------------------------------------------------
def forced_fit(kv, K=8, D=64, N=6000, iters=12):
    from bayesml_amd import gaussianmixture as gm
    from oracle import gmm_vb_oracle as orc
    x = orc.synth_gmm(K, D, N, np.float32)
    with env(kv):
        m = gm.LearnModel(K, D, seed=0, device=dev(), verbose=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.update_posterior(x, max_itr=iters, num_init=1, tolerance=0.0)
    hn = dict(m.get_hn_params(), s_mats=m.s_mats, ns=m.ns)
    return hn, m._engine.pass_counts(), m._engine.work()


def test_delta_lists_of_a_forced_fit():
    fits = {"runs=1": switches(1), "runs=3": switches(3), "device": switches(None),
            "no cache": switches(None, GMMVB_DEBUG="1", GMMVB_MSTEP_CACHE="0"),
            "dense M": {"GMMVB_ESTEP_PRUNE": "0", "GMMVB_MSTEP_SPARSE": "0"}}
    out = {tag: forced_fit(kv) for tag, kv in fits.items()}
    for tag in ("runs=1", "runs=3", "device", "no cache"):
        assert out[tag][1]["mstep_list"] >= 10, (tag, out[tag][1])
    assert out["device"][2]["settled_rows"] > 0, out["device"][2]            # rows settled: the delta lists had entries
    assert out["no cache"][2]["accumulated"] == out["no cache"][2]["active"], out["no cache"][2]      # (nothing held back)
    assert out["dense M"][1]["mstep_list"] == 0, out["dense M"][1]
    tags = sorted(out)
    for i, a in enumerate(tags):
        for b in tags[i + 1:]:
            for key, val in out[a][0].items():
                err = rel_err(val, out[b][0][key])
                print("mlist-runs delta", a, "against", b, key, err)
                assert err < (1e-5 if key == "s_mats" else 1e-6), (a, b, key)
