"""Tile-level shortcuts for tiles of 256 rows that are settled throughout (csrc/workspace.h: tile state; records.h:
rec_finish_kernel and settled_mask_kernel take them, rec_sweep_kernel and rec_proof_decide_kernel keep the count they rest
on) must not change a bit.

Every scenario drives the engine the way update_posterior does (K-side update -> drift hint -> data pass, as
tests/test_gpu_sparse_parity.py does) with the pruned path forced, twice on identical seeded inputs: once with
GMMVB_QUIET_TILES=0 and once with the default.  After EVERY pass the two runs must agree bit for bit in the statistics
block, the responsibilities of all rows, the hard assignments, sparsity(), work(), pass_counts() and every term of the
lower bound; the default run is also held to the oracle with the tolerances of the sparse-parity suite (responsibilities
1e-9 absolute, ns 1e-10 and s 1e-9 relative).

Shapes: D = 64, N = 256 * 9 + 37 rows (ten tiles, the last one ragged), at most 12 passes per scenario.  Every run
starts from the posterior of the true labels instead of the subsampled start: from that one the first iterations at
these sizes keep six or seven broad components active per row (measured at K = 16), the policy never leaves the bound
pass and no kernel with a shortcut is launched.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
from oracle import gmm_vb_oracle as orc

pytestmark = pytest.mark.gpu

D, N = 64, 256 * 9 + 37
TILES = (N + 255) // 256


class switches:
    """The environment a workspace is created under (its switches are read once, at creation)."""

    def __init__(self, quiet):
        self.kv = {"GMMVB_ESTEP_PRUNE": "force"}
        if not quiet:
            self.kv["GMMVB_QUIET_TILES"] = "0"

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("GMMVB_ESTEP_PRUNE", "GMMVB_QUIET_TILES")}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def labelled(mu, z):
    rng = np.random.default_rng(20250712)
    return (mu[z] + rng.standard_normal((len(z), D))).astype(np.float32), z


def far_apart(K):
    """The benchmark's recipe: means 2 * randn in 64 dimensions, some 22 standard deviations apart - every row settles."""
    rng = np.random.default_rng(20250711)
    return labelled(2.0 * rng.standard_normal((K, D)), rng.integers(0, K, N))


def partly_overlapping(K):
    """K = 8, rows in cluster order so that tiles are pure: tile 0 isolated | tiles 1-2 a pair of clusters 12 standard
    deviations apart (ln of the density ratio 72 + 12 z against the 55.45 of 2^-80: about one row in twelve keeps both
    components) | tiles 3-4 isolated | tiles 5-6 a pair 13 apart (84.5 + 13 z: one row in eighty) | tile 7 isolated |
    tile 8 and the ragged tile 9: the two outer isolated clusters.  Six tiles go quiet next to four that never do."""
    assert K == 8
    rng = np.random.default_rng(20250711)
    mu = 2.0 * rng.standard_normal((K, D))
    for a, b, dist in ((1, 2, 12.0), (5, 6, 13.0)):
        step = rng.standard_normal(D)
        mu[b] = mu[a] + dist * step / np.linalg.norm(step)
    return labelled(mu, np.concatenate([np.repeat(np.arange(K), 256), rng.choice([0, 7], N - K * 256)]))


class Run:
    """One engine over x under one setting of the switch; a snapshot of everything observable after every pass."""

    def __init__(self, x, z, K, quiet):
        from bayesml_amd import _kside
        from bayesml_amd import gaussianmixture as gm
        self.ks, self.K, self.quiet = _kside, K, quiet
        dev = torch.device("cuda", 0)
        with switches(quiet):
            self.m = gm.LearnModel(K, D, seed=0, device=dev, verbose=False)
            self.eng, self.xd = self.m._open(x)
        self.prior = self.m._prior_tensors(dev)
        self.q = None
        self.s = torch.zeros(K, D, D, dtype=torch.float64, device=dev)
        self.snaps, self.posts = [], []
        # the posterior of the true labels
        x64 = torch.from_numpy(x.astype(np.float64)).to(dev)
        r = torch.nn.functional.one_hot(torch.from_numpy(z), K).to(dev, torch.float64)
        ns = r.sum(dim=0)
        x_bar = (r.T @ x64) / ns[:, None]
        c = x64[:, None, :] - x_bar[None, :, :]
        s = torch.einsum("nk,nki,nkj->kij", r, c, c) / ns[:, None, None]
        self.step(_kside.update_q(self.prior, ns, x_bar, s), hint=None)

    def step(self, q, hint="drift", summary=True):
        """One data pass under q; hint "drift": the drift hint of the update self.q -> q, with the driver's one-number
        summary of it (below 0.5 the policy makes the bounds afresh) or without (the sweep carries whatever the drift);
        None: no hint (a bound pass)."""
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
        """self.q with component k_from's mean moved `share` of the way to k_to's."""
        q = self.q
        m = q.m.clone()
        m[k_from] = q.m[k_from] + share * (q.m[k_to] - q.m[k_from])
        return self.ks.features(self.ks.PostT(q.alpha.clone(), m, q.kappa.clone(), q.nu.clone(), q.w_inv.clone()))

    def settled(self, i):
        return self.snaps[i]["work"]["settled_rows"]

    def swept(self, i):
        return self.snaps[i]["info"].startswith("estep_sweep_bounds")


def everything_settles(run):
    run.vb(9)                   # (two or three passes settle every row; the shortcuts are taken in each pass after the next)


def quiet_loose_quiet(run):
    run.vb(4)
    keep = run.q
    run.step(run.moved(0, 1, 0.98), summary=False)      # rows of quiet tiles get candidates, go through the proof round, come loose
    run.vb(2)
    run.step(keep, summary=False)               # back to where the rows had settled
    run.vb(3)


def flag_cleared(run):
    run.vb(4)
    run.step(run.ks.update_q(run.prior, run.ns, run.x_bar, run.s), hint=None)      # no drift hint: a bound pass
    run.vb(2)
    run.eng.responsibilities()                  # (every pass is followed by read-outs; one more for good measure)
    run.eng.ln_rho()
    run.vb(3)


SCENARIOS = {
    "everything_settles": (6, far_apart, everything_settles),
    "two_mask_words": (70, far_apart, everything_settles),
    "quiet_loose_quiet": (6, far_apart, quiet_loose_quiet),
    "flag_cleared": (6, far_apart, flag_cleared),
    "partly_quiet": (8, partly_overlapping, everything_settles),
}


def oracle_post(q):
    n = lambda t: t.detach().cpu().numpy().copy()   # noqa: E731
    o = orc.Posterior(alpha=n(q.alpha), m=n(q.m), kappa=n(q.kappa), nu=n(q.nu), w=n(q.w), w_inv=n(q.w_inv))
    o.refresh_pi()
    o.refresh_lambda()
    return o


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


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_shortcuts_change_no_bit(name):
    K, make, play = SCENARIOS[name]
    x, z = make(K)
    runs = []
    for quiet in (False, True):
        run = Run(x, z, K, quiet)
        play(run)
        runs.append(run)
    off, on = runs
    assert len(on.snaps) == len(off.snaps) <= 12
    print(name, [(s["info"].split(" ")[0], int(s["work"]["settled_rows"]), int(s["work"]["proof_pairs"])) for s in on.snaps])
    for i, (a, b) in enumerate(zip(off.snaps, on.snaps)):
        for key in a:
            assert same_bits(a[key], b[key]), (name, "pass", i, key)
    # the default run against the oracle after every pass that lived on carried bounds (as the sparse-parity suite does:
    # the first pass runs under the subsampled start, ln rho of the order 1e7, and is no sweep)
    x64 = x.astype(np.float64)
    assert sum(on.swept(i) for i in range(len(on.snaps))) >= 3
    for i, (snap, q) in enumerate(zip(on.snaps, on.posts)):
        if not on.swept(i):
            continue
        st = orc.data_pass(x64, oracle_post(q))
        ns, _h, a, B = on.eng.split_stats(torch.from_numpy(snap["stats"]))
        assert np.max(np.abs(snap["r"] - st.r)) < 1e-9, (name, i)
        assert rel_err(ns.numpy(), st.ns) < 1e-10, (name, i)
        assert np.array_equal(snap["z"], snap["r"].argmax(axis=1)), (name, i)
    last = len(on.snaps) - 1
    assert on.swept(last)
    assert rel_err(on.s.cpu().numpy(), orc.data_pass(x64, oracle_post(on.posts[last])).s) < 1e-9, name
    # what each scenario is there for really happened (in both runs: the snapshots are equal)
    if name in ("everything_settles", "two_mask_words"):
        assert all(on.swept(i) and on.settled(i) == N for i in range(last - 3, last + 1)), [on.settled(i) for i in range(last + 1)]
    if name == "quiet_loose_quiet":
        assert on.settled(4) == N and on.swept(5) and on.settled(5) < N, [on.settled(i) for i in range(last + 1)]
        assert on.snaps[5]["work"]["proof_pairs"] > 0
        assert on.swept(last) and on.settled(last) == N, [on.settled(i) for i in range(last + 1)]
    if name == "flag_cleared":
        assert on.settled(4) == N and on.snaps[5]["counts"]["estep_bound"] == on.snaps[4]["counts"]["estep_bound"] + 1
        assert on.swept(last) and on.settled(last) == N
    if name == "partly_quiet":
        assert all(on.swept(i) and 0.5 * N < on.settled(i) < N for i in range(last - 3, last + 1)), [on.settled(i) for i in range(last + 1)]
    for run in runs:
        run.eng.close()


@pytest.mark.parametrize("quiet", [True, False])
def test_debug_line_counts_the_quiet_tiles(quiet):
    """The shortcut is really taken: a fresh process runs "everything settles" with GMMVB_DEBUG=2; the line every E-step
    prints reports, for the pass before it, every tile quiet in the last passes - and no tile state at all (-1) when the
    switch is off."""
    child_env = dict(os.environ, GMMVB_DEBUG="2")
    child_env.pop("GMMVB_QUIET_TILES", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "1" if quiet else "0"], env=child_env,
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = [tuple(int(v) for v in m) for m in re.findall(r"\[gmmvb\] estep: .* quiet=(-?\d+)/(\d+) skipped=(-?\d+)", r.stderr)]
    assert len(seen) == 10, r.stderr[-2000:]
    if quiet:       # (quiet after the sweep's selection, of the tiles, taken the short way through rec_finish_kernel)
        assert seen[-4:] == [(TILES, TILES, TILES)] * 4, seen
    else:
        assert all(s == (-1, TILES, -1) for s in seen), seen


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    run = Run(*far_apart(6), 6, sys.argv[2] == "1")
    everything_settles(run)
    run.eng.close()
