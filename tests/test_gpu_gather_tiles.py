"""estep_gather_dev_f64 (bayesml_amd/csrc/estep.h) hands its persistent workgroups ranges of workgroup tiles (8 waves x 16 NB
list entries), not whole chunks of kGatherTiles tiles: a range may start and end inside a chunk, and a chunk, or a component's
list, may be shared by several workgroups.  Every pair's ln rho comes from its own MFMA column with the operations of the dense
kernels, so whoever evaluates a listed pair, and whatever else shares its tile, the value is the dense E-step's bit for bit.

One forced pruned E-step (GMMVB_ESTEP_PRUNE=force, GMMVB_GATHER_EXIT=0: every listed pair evaluated in full) against one
dense E-step of a twin workspace under the same parameters.  A pair of the pruned pass is either exact - the dense bits - or
shown irrelevant: then it holds an upper bound of ln rho at least 80 ln 2 below the row's log-sum (tests/test_gpu_sparse.py
states the same property to rounding).  The exact pairs per component are counted from the output, so each case also holds
its own premise: the list lengths that put the range edges where the case wants them.

Tile and chunk: 128 and 1024 entries at D = 128 (NB = 1), 256 and 2048 at D = 64 (NB = 2), f32 rows.  The launch has
2 x (compute units) workgroups - 512 on the 256 units of an MI355X.

* far-apart clusters of chosen sizes, parameters at their means: component k's list is cluster k.  A few dozen tiles over
  hundreds of workgroups - every live tile is a range of its own inside a chunk; lists of one entry (first, in the middle),
  a list one chunk and a few entries long, a list that ends inside its third chunk.
* five near-identical components over one cloud: every pair is a candidate, 1 175 (D = 128) or 590 (D = 64) tiles - ranges
  of one to three tiles that cross chunk and component boundaries at no multiple of kGatherTiles.

The early-exit form (a row's candidates leave once a partial bound lies below the row's threshold) decides per wave tile, and
the wave tiles are the same entries as before: its output was compared, bit for bit, with the parent commit's library over
these cases in the session that made the change (profiles/mlist_runs.md); here it must reproduce itself and stay sound."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 5
KEYS = ("GMMVB_ESTEP_PRUNE", "GMMVB_GATHER_EXIT", "GMMVB_MSTEP_SPARSE")


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


def far_apart(D, sizes, seed):
    """Cluster k has sizes[k] rows around a mean 8 standard deviations per feature from the others; rows shuffled."""
    rng = np.random.default_rng(seed)
    mu = 8.0 * rng.standard_normal((K, D))
    z = rng.permutation(np.repeat(np.arange(K), sizes))
    return (mu[z] + rng.standard_normal((len(z), D))).astype(np.float32), mu, z


def one_cloud(D, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, D)).astype(np.float32), 0.01 * rng.standard_normal((K, D)), None


def features(mu, N):
    """Unit precisions around the means `mu`, equal weights (as tests/test_gpu_mstep_plan.py's f64 list case)."""
    from bayesml_amd import _kside
    D = mu.shape[1]
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev())   # noqa: E731
    return _kside.features(_kside.PostT(t(np.full(K, N / K)), t(mu), t(np.full(K, 100.0)), t(np.full(K, D + 100.0)),
                                        t(np.tile((D + 100.0) * np.eye(D), (K, 1, 1)))))


def ln_rho_of(x, mu, switches):
    """ln rho [N][K] of one E-step of a fresh workspace, its gather launches and its launch line."""
    from bayesml_amd._engine import DataPass
    N, D = x.shape
    xd = torch.from_numpy(x).to(dev())
    qd = features(mu, N)
    with env(switches):
        eng = DataPass(K, D, xd.dtype, N, dev())
    eng.set_pivot(xd[:4096].to(torch.float64).mean(dim=0))
    eng.prepare_rows(xd)
    eng.set_params(qd.c, qd.m, qd.u)
    eng.estep(xd)
    out = eng.ln_rho().cpu().numpy()
    gathers, info = eng.pass_counts()["estep_gather"], eng.launch_info
    eng.close()
    return out, gathers, info


DENSE = {"GMMVB_ESTEP_PRUNE": "0", "GMMVB_MSTEP_SPARSE": "0"}
FULL = {"GMMVB_ESTEP_PRUNE": "force", "GMMVB_GATHER_EXIT": "0"}
EXIT = {"GMMVB_ESTEP_PRUNE": "force"}

CASES = {
    # name: (D, builder, argument, what the exact pairs per component must be)
    "edges-128": (128, far_apart, [1, 2900, 1, 1500, 1030], "sizes"),
    "edges-64": (64, far_apart, [1, 5000, 1, 2049, 2100], "sizes"),
    "cloud-128": (128, one_cloud, 30_080, "all"),
    "cloud-64": (64, one_cloud, 30_208, "all"),
}
_dense = {}


def case(name):
    D, build, arg, _ = CASES[name]
    x, mu, z = build(D, arg, 20260 + D)
    if name not in _dense:          # the reference of a case is computed once and left alone
        la, gathers, info = ln_rho_of(x, mu, DENSE)
        assert gathers == 0 and "_bound" not in info, info
        la.setflags(write=False)
        _dense[name] = la
    return x, mu, z, _dense[name]


def exact_or_irrelevant(la, lb):
    exact = la == lb
    mx = la.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(la - mx).sum(axis=1, keepdims=True))
    rest = ~exact
    assert np.all(lb[rest] >= la[rest]), "a pair that is not the dense E-step's bits lies below them: it is no upper bound"
    assert np.all((lb <= lse - 55.4)[rest]), "a pair that is not the dense E-step's bits is not irrelevant"   # 80 ln 2 = 55.45
    return exact


@pytest.mark.parametrize("name", sorted(CASES))
def test_listed_pairs_are_the_dense_bits(name):
    x, mu, z, la = case(name)
    lb, gathers, info = ln_rho_of(x, mu, FULL)
    assert gathers >= 1 and "_bound" in info, info
    exact = exact_or_irrelevant(la, lb)
    per_component = exact.sum(axis=0)
    print("gather-tiles", name, "exact pairs per component", per_component.tolist(), "of", len(x), "rows |", info)
    if CASES[name][3] == "all":
        assert exact.all()
    else:
        # each row's own pair was listed and evaluated, and the lists are the clusters: the lengths the case is about
        assert exact[np.arange(len(z)), z].all()
        assert per_component.tolist() == CASES[name][2]


@pytest.mark.parametrize("name", sorted(CASES))
def test_early_exit_form_is_sound_and_repeats(name):
    x, mu, z, la = case(name)
    first, gathers, info = ln_rho_of(x, mu, EXIT)
    again, _, _ = ln_rho_of(x, mu, EXIT)
    assert gathers >= 1 and "_bound" in info, info
    assert np.array_equal(first, again)
    exact = exact_or_irrelevant(la, first)
    print("gather-tiles", name, "early-exit form: exact pairs per component", exact.sum(axis=0).tolist())
    if z is not None:
        assert exact[np.arange(len(z)), z].all()
