"""The carried sweep (csrc/records.h: rec_sweep_kernel) lets a workgroup go through a run of R consecutive tiles of 256 rows,
one after the other, with the per-component constants and the zeroed counters set up once per run and ONE addition to the
opened-columns counter per run instead of one per tile.  Per row and per column nothing is computed differently, so
whatever the run length, every pass must leave the same bits - the counter (work()["sweep_share"]) included.

Every case drives the engine the way update_posterior does (K-side update -> drift hint -> data pass, as
tests/test_gpu_quiet_tiles.py does) with the pruned path forced, once per compiled run length on identical inputs:
GMMVB_SWEEP_RUN=1 (a tile per workgroup, the order of work before the runs), 2 and 4 (a developer switch: behind
GMMVB_DEBUG, read when the workspace is created).  After EVERY pass the runs must agree bit for bit in the statistics
block, the responsibilities of all rows, the hard assignments, sparsity(), work(), pass_counts(), the launch line and
every term of the lower bound (which holds the sum of the rows' log-normalisers).

Shapes: K = 64, D = 128, f32 rows in cluster order; N such that the tile count is 1, R - 1, R, R + 1 and 2 R + 1 for
R = 2 and R = 4 - 1, 2, 3, 4, 5, 9 tiles - with the last tile ragged (219 rows short) and, in a second set, full.  One case
each at K = 65 and K = 130 (two and three mask words; at three the library keeps a tile per workgroup, whatever the switch),
D = 64.  Every run starts from the posterior of the true labels: its first pass is a bound pass, the first sweep behind it
finds the tile state void (tmeta_reset: every column opened), the sweeps after it carry that state.
The rows come from six clusters laid out one after the other (the other components stay at the prior).
* loose: after four passes component 2's mean moves 98 % of the way to component 3's: the rows of both - rows 342 to 682
  of 1024, in the second and third of four tiles, so in the second tile of a run for R = 2 and R = 4 - get candidates, go
  through the proof round and come loose.
* nan: one row in the last tile of a run is NaN - row 1000 of four full tiles (tile 3: the last of a run for both R), and
  row 1400 of six (tile 5: the last tile of R = 4's short second run, tiles 4 and 5).  The parameters are those of the
  clean rows' trajectory and the pivot is the clean rows' mean (the driver's own pivot, the mean of the first 4096 rows,
  would be NaN and with it every row: no pass would ever leave the bound kernel), so the sweeps go on and meet the row -
  no reference value, every pair a candidate, an overflow row - in every pass.
K = 130 only pins that the switch is ignored above K = 128.  Nothing observable on the GPU tells the run lengths apart (the
launch line is the same by design): that the switch reaches the launch is held by tests/test_sweep_run.py on the host.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RUNS = (1, 2, 4)
KEYS = ("GMMVB_ESTEP_PRUNE", "GMMVB_DEBUG", "GMMVB_SWEEP_RUN")


class switches:
    """The environment a workspace is created under (its switches are read once, at creation)."""

    def __init__(self, run):
        self.kv = {"GMMVB_ESTEP_PRUNE": "force", "GMMVB_DEBUG": "1", "GMMVB_SWEEP_RUN": str(run)}

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


CLUSTERS = 6


def rows_in_cluster_order(K, D, N, seed=20260720):
    """The benchmark's recipe (means 2 * randn: some 22 to 32 standard deviations apart) for CLUSTERS clusters, N rows dealt
    evenly over them and laid out cluster after cluster: cluster c's rows are rows c N / 6 to (c + 1) N / 6, regrouped or
    not.  The other K - 6 components own no row: they start from the prior and stay there (with a few rows per component
    the posteriors at these N are broad, every row keeps several components and the policy never leaves the bound pass)."""
    rng = np.random.default_rng(seed)
    mu = 2.0 * rng.standard_normal((K, D))
    z = np.sort(np.arange(N) % CLUSTERS)
    return (mu[z] + rng.standard_normal((N, D))).astype(np.float32), z


class Run:
    """One engine over x under one run length; a snapshot of everything observable after every pass."""

    def __init__(self, x, z, K, run, start_x=None):
        from bayesml_amd import _kside
        from bayesml_amd import gaussianmixture as gm
        D = x.shape[1]
        self.ks, self.K = _kside, K
        dev = torch.device("cuda", 0)
        with switches(run):
            self.m = gm.LearnModel(K, D, seed=0, device=dev, verbose=False)
            self.eng, self.xd = self.m._open(x)
        if start_x is not None:         # the clean rows' pivot (see "nan" above)
            self.eng.set_pivot(torch.from_numpy(start_x[:4096].astype(np.float64)).to(dev).mean(dim=0))
            self.eng.prepare_rows(self.xd)
        self.prior = self.m._prior_tensors(dev)
        self.q = None
        self.s = torch.zeros(K, D, D, dtype=torch.float64, device=dev)
        self.snaps, self.posts = [], []
        # the posterior of the true labels (of the clean rows, where x has a NaN row)
        x64 = torch.from_numpy((x if start_x is None else start_x).astype(np.float64)).to(dev)
        r = torch.nn.functional.one_hot(torch.from_numpy(z), K).to(dev, torch.float64)
        ns = r.sum(dim=0)
        x_bar = (r.T @ x64) / ns.clamp(min=1.0)[:, None]
        c = x64[:, None, :] - x_bar[None, :, :]
        s = torch.einsum("nk,nki,nkj->kij", r, c, c) / ns.clamp(min=1.0)[:, None, None]
        self.step(_kside.update_q(self.prior, ns, x_bar, s), hint=None)

    def step(self, q, hint="drift", summary=True):
        if hint == "drift":
            h = self.m._drift_hint(self.eng, self.xd, self.q, q)
            assert h is not None
            hint = (*h, float((h[0] - h[1] / 30.0).min())) if summary else tuple(h)
        self.m._give_params(self.eng, q, hint)
        stats = self.eng.estep_mstep(self.xd).clone()
        ns, h, a, B = self.eng.split_stats(stats)
        self.ns = ns
        self.x_bar, self.s = self.ks.moments_from_stats(ns, a, B, self.eng.pivot, self.s)
        self.q = q
        terms = self.ks.lower_bound(self.prior, q, ns, self.x_bar, self.s, h.sum())
        self.snaps.append(dict(stats=stats.cpu().numpy(), r=self.eng.responsibilities().cpu().numpy(),
                               z=self.eng.argmax().cpu().numpy(), sparsity=self.eng.sparsity(), work=self.eng.work(),
                               counts=self.eng.pass_counts(), info=self.eng.launch_info,
                               bound={k: float(v) for k, v in terms.items()}))
        self.posts.append(q)

    def vb(self, passes):
        for _ in range(passes):
            self.step(self.ks.update_q(self.prior, self.ns, self.x_bar, self.s))

    def moved(self, k_from, k_to, share):
        q = self.q
        m = q.m.clone()
        m[k_from] = q.m[k_from] + share * (q.m[k_to] - q.m[k_from])
        return self.ks.features(self.ks.PostT(q.alpha.clone(), m, q.kappa.clone(), q.nu.clone(), q.w_inv.clone()))

    def settled(self, i):
        return self.snaps[i]["work"]["settled_rows"]

    def swept(self, i):
        return self.snaps[i]["info"].startswith("estep_sweep_bounds")


def same_bits(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(u, v) for u, v in zip(a, b))
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def all_run_lengths(name, x, z, K, play, start_x=None):
    """play(run) for every run length; every snapshot of every pass equal to the one-tile form's.  Returns that form's run."""
    runs = []
    for length in RUNS:
        run = Run(x, z, K, length, start_x)
        play(run)
        runs.append(run)
    one = runs[0]
    print(name, [(s["info"].split(" ")[0], int(s["work"]["settled_rows"]), int(s["work"]["proof_pairs"])) for s in one.snaps])
    for length, run in zip(RUNS[1:], runs[1:]):
        assert len(run.snaps) == len(one.snaps)
        for i, (a, b) in enumerate(zip(one.snaps, run.snaps)):
            for key in a:
                assert same_bits(a[key], b[key]), (name, "run length", length, "pass", i, key)
    for run in runs[1:]:
        run.eng.close()
    return one


def carried(run, at_least):
    """The passes behind the first are carried sweeps: the first of them under a void tile state, the others carrying it."""
    sweeps = [i for i in range(len(run.snaps)) if run.swept(i)]
    assert len(sweeps) >= at_least, [s["info"] for s in run.snaps]
    return sweeps


TILE_COUNTS = (1, 2, 3, 4, 5, 9)


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "full"])
@pytest.mark.parametrize("tiles", TILE_COUNTS)
def test_every_run_length_leaves_the_same_bits(tiles, ragged):
    K, D, N = 64, 128, 256 * tiles - (219 if ragged else 0)
    x, z = rows_in_cluster_order(K, D, N)
    one = all_run_lengths(f"sweep-runs tiles={tiles} ragged={ragged}", x, z, K, lambda run: run.vb(5))
    sweeps = carried(one, 3)
    assert one.settled(len(one.snaps) - 1) > 0            # (rows settled: the sweep took their reference from dlock)
    assert all(0.0 < one.snaps[i]["work"]["sweep_share"] <= 1.0 for i in sweeps), [s["work"] for s in one.snaps]
    one.eng.close()


@pytest.mark.parametrize("K", [65, 130])
def test_two_and_three_mask_words(K):
    D, N = 64, 256 * 5 - 219
    x, z = rows_in_cluster_order(K, D, N)
    one = all_run_lengths(f"sweep-runs K={K}", x, z, K, lambda run: run.vb(5))
    carried(one, 3)
    one.eng.close()


def test_a_settled_row_comes_loose_in_the_second_tile_of_a_run():
    K, D, N = 64, 128, 256 * 4

    def play(run):
        run.vb(4)
        keep = run.q
        run.step(run.moved(2, 3, 0.98), summary=False)
        run.vb(2)
        run.step(keep, summary=False)
        run.vb(2)

    x, z = rows_in_cluster_order(K, D, N)
    one = all_run_lengths("sweep-runs loose", x, z, K, play)
    carried(one, 5)
    assert one.swept(5) and one.settled(5) < one.settled(4), [one.settled(i) for i in range(len(one.snaps))]
    assert one.snaps[5]["work"]["proof_pairs"] > 0
    one.eng.close()


@pytest.mark.parametrize("tiles,row", [(4, 1000), (6, 1400)])
def test_a_nan_row_in_the_last_tile_of_a_run(tiles, row):
    K, D, N = 64, 128, 256 * tiles
    x, z = rows_in_cluster_order(K, D, N)
    clean = Run(x, z, K, 1)
    clean.vb(5)
    posts = clean.posts[1:]
    clean.eng.close()
    bad = x.copy()
    bad[row] = np.nan

    def play(run):          # the clean rows' parameters, pass after pass
        for q in posts:
            run.step(q)

    one = all_run_lengths(f"sweep-runs nan tiles={tiles}", bad, z, K, play, start_x=x)
    sweeps = carried(one, 3)
    for i in sweeps:        # the other rows are none the worse for it
        r = one.snaps[i]["r"]
        print("sweep-runs nan row", i, r[row][:8])
        assert not np.isnan(np.delete(r, row, axis=0)).any(), i
    one.eng.close()
