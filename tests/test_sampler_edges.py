"""CPU side of the sampler edge tests: the exact oracle, its bound and the chain checker of tests/sampler_exact.py are
themselves put to the test here, on the cases of tests/sampler_cases.py that tests/test_gpu_sampler_edges.py runs on the
kernels.

* NumPy's float64 sum of the exact normals is within 2 B_j of the exact oracle on every emission case - a bound that a
  correct float64 evaluation misses would be no bound - and the whole float64 restatement (oracle/sampler_oracle.py),
  whose normals carry an ABSOLUTE angle error the kernel's do not, is within 2 B_j(host) (sampler_exact's docstring);
* the vectorised chain checker accepts the sequential recursion and rejects three kinds of planted error, among them the
  two a wrong carry between chunks or groups produces;
* every chain case's chunk maps do not coalesce (the precondition under which the carry decides anything);
* the hand-picked tolerance of tests/test_samplers.py, 2e-13 (1 + |x|), is no bound away from unit scale: too tight for
  NumPy itself at covariance scale 1e8, loose enough for normals rounded to float32 at 1e-14.
Every test prints its worst |error| / B_j (``-s`` shows them; profiles/sampler_tests.md records them).
"""
import numpy as np
import pytest

import sampler_cases as sc
import sampler_exact as sx
from oracle import sampler_oracle as so

EMIT = {c.name: c for c in sc.emission_cases()}


def test_exact_normals_are_the_host_stream_and_window():
    """The mpmath normals agree with the float64 restatement to float64 rounding of a rounded angle (a loose, absolute
    statement: the sharp one is the device's, relative) and a window at row0 is the same rows of a longer draw."""
    for D in (1, 3, 4, 5, 8):
        e = sx.normals(77, 0, 40, D)
        assert e.dtype == np.longdouble and e.shape == (40, D)
        assert np.max(np.abs(so.normals(77, 0, 40, D) - e.astype(np.float64))) < 1e-14
        assert np.array_equal(sx.normals(77, 29, 11, D), e[29:])
    big = 2 ** 40 + 3
    assert np.max(np.abs(so.normals(5, big, 9, 7) - sx.normals(5, big, 9, 7).astype(np.float64))) < 1e-14


@pytest.mark.parametrize("name", list(EMIT))
def test_numpy_restatement_is_within_the_bound(name):
    c = EMIT[name]
    ex = sx.Emissions(c.z, c.mu, c.a, c.seed, c.row0)
    r = ex.ratio(c.mu[c.z] + np.einsum("ni,nij->nj", ex.e64, c.a[c.z]))
    rh = ex.ratio(so.emissions(c.z, c.mu, c.a, c.seed, c.row0), host=True)
    print(f"\n[sampler-edges] numpy {name}: worst |error| / B_j = {r:.3f} with the exact normals, "
          f"|error| / B_j(host) = {rh:.3f} with its own (allowed 2)")
    assert r <= 2.0 and rh <= 2.0


def test_bound_rejects_a_subtly_wrong_emission():
    """What 2 B_j still sees: one normal off by 2^-40 relative, one product dropped at the end of the longest sum."""
    c = EMIT["dispatch-D33"]
    ex = sx.Emissions(c.z, c.mu, c.a, c.seed)
    eps = so.normals(c.seed, 0, c.z.shape[0], c.D)
    bent = eps.copy()
    bent[:, 20] *= 1.0 + 2.0 ** -40
    assert ex.ratio(c.mu[c.z] + np.einsum("ni,nij->nj", bent, c.a[c.z])) > 2.0
    short = c.a.copy()
    short[:, -1, 0] = 0.0
    assert ex.ratio(c.mu[c.z] + np.einsum("ni,nij->nj", eps, short[c.z])) > 2.0


def test_old_tolerance_is_not_a_bound():
    """Covariances x 1e8: NumPy's own float64 sum misses 2e-13 (1 + |x|) where an entry cancels, and is within 2 B_j
    (2 B_j(host) with the restatement's own normals).
    Covariances x 1e-14: a stand-in whose normals are rounded to float32 passes 2e-13 (1 + |x|) and misses 2 B_j."""
    c = EMIT["cov-x1e+08"]
    ex = sx.Emissions(c.z, c.mu, c.a, c.seed)
    x = c.mu[c.z] + np.einsum("ni,nij->nj", ex.e64, c.a[c.z])
    old, new = ex.old_ratio(x), ex.ratio(x)
    print(f"\n[sampler-edges] covariance x 1e8, NumPy float64 sum: |error| / (2e-13 (1 + |x|)) = {old:.2f}, |error| / B_j = {new:.3f}")
    assert old > 1.0 and new <= 2.0
    x = so.emissions(c.z, c.mu, c.a, c.seed)
    old, new = ex.old_ratio(x), ex.ratio(x, host=True)
    print(f"[sampler-edges] covariance x 1e8, NumPy restatement: |error| / (2e-13 (1 + |x|)) = {old:.2f}, |error| / B_j(host) = {new:.3f}")
    assert old > 1.0 and new <= 2.0
    c = sc.covariance_scaled(1e-14)
    ex = sx.Emissions(c.z, c.mu, c.a, c.seed)
    eps32 = so.normals(c.seed, 0, c.z.shape[0], c.D).astype(np.float32).astype(np.float64)
    x = c.mu[c.z] + np.einsum("ni,nij->nj", eps32, c.a[c.z])
    old, new = ex.old_ratio(x), ex.ratio(x)
    print(f"[sampler-edges] covariance x 1e-14, float32 normals: |error| / (2e-13 (1 + |x|)) = {old:.2e}, |error| / B_j = {new:.3g}")
    assert old <= 1.0 and new > 2.0


# ---- chains ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CHAINS))
def test_checker_accepts_the_recursion_and_maps_do_not_coalesce(name):
    pi, a = sc.CHAINS[name]()
    for T in sc.CHAIN_T:
        seed = sc.chain_seed(name, T)
        z = so.markov_chain(pi, a, seed, T)
        assert sx.chain_is_the_recursion(z, pi, a, seed), T
        maps = sx.chunk_maps(pi, a, seed, T)
        assert 2 * sx.nonconstant_maps(maps[1:]) >= maps.shape[0] - 1, T
        # the host's statement of the device's plan: composing the maps and replaying the chunks IS the recursion
        if T in (257, 513, 65536 + 257):
            assert np.array_equal(sx.chain_from_maps(pi, a, seed, T, maps), z), T


@pytest.mark.parametrize("name", sc.LONG_CHAINS)
def test_long_chain_maps_do_not_coalesce(name):
    pi, a = sc.CHAINS[name]()
    maps = sx.chunk_maps(pi, a, sc.chain_seed(name, sc.LONG_T), sc.LONG_T)
    non, of = sx.nonconstant_maps(maps[1:]), maps.shape[0] - 1
    # ... but these two forget their start within a group of 65536 steps: every full group's map is constant, which is why
    # sampler_cases.GROUP_CHAINS exist
    assert sx.nonconstant_maps(sx.group_maps(maps)[:-1]) == 0
    print(f"\n[sampler-edges] {name} T = 2^24 + 1029: {non} of {of} chunk maps after the first are non-constant")
    assert of == 65540 and 2 * non >= of


@pytest.mark.parametrize("name,T", [(name, T) for name, Ts in sc.GROUP_CHAINS.items() for T in Ts])
def test_group_maps_do_not_coalesce(name, T):
    """The chains that test thread 0's chaining of the groups: at least half of the group maps after the first are
    non-constant too."""
    pi, a = sc.CHAINS[name]()
    gm = sx.group_maps(sx.chunk_maps(pi, a, sc.chain_seed(name, T), T))
    assert gm.shape[0] >= 4 and 2 * sx.nonconstant_maps(gm[1:]) >= gm.shape[0] - 1


@pytest.mark.parametrize("name", ["shift-5", "shift-257", "two-classes", "sticky-2", "cycle-jumps-5", "absorbing"])
def test_checker_rejects_planted_errors(name):
    pi, a = sc.CHAINS[name]()
    K, T = pi.shape[0], 65536 + 257
    seed = sc.chain_seed(name, T)
    z = so.markov_chain(pi, a, seed, T)
    assert sx.chain_first_mismatch(z, pi, a, seed) == -1
    # one state changed in the middle of a chunk
    for t in (100, 256 * 7 + 128, T - 1):
        bad = z.copy()
        bad[t] = (bad[t] + 1) % K
        assert sx.chain_first_mismatch(bad, pi, a, seed) == t
    out = z.copy()
    out[300] = K
    assert sx.chain_first_mismatch(out, pi, a, seed) == 300
    # correct GIVEN a wrong carried state, from a chunk border and from the group border on
    for t0 in (256, 256 * 9, 65536):
        wrong = [s for s in range(K) if s != z[t0 - 1]][:3]
        tails = [sx.recursion_from(pi, a, seed, t0, T, s) for s in wrong]
        tails = [t for t in tails if t[0] != z[t0]]               # (a wrong state that merges at once plants nothing)
        assert tails, (name, t0)
        bad = np.concatenate([z[:t0], tails[0]])
        assert sx.chain_first_mismatch(bad, pi, a, seed) == t0


def test_swapped_maps_are_seen_where_maps_do_not_commute():
    """The plan of the device with two adjacent chunk maps swapped before they are composed.  Rotations commute, so the
    swap plants nothing on the pure shifts; this chain's maps do not."""
    pi, a = sc.CHAINS["cycle-jumps-5"]()
    T = 65536 + 257
    seed = sc.chain_seed("cycle-jumps-5", T)
    z = so.markov_chain(pi, a, seed, T)
    maps = sx.chunk_maps(pi, a, seed, T)
    seen = 0
    for c in range(1, maps.shape[0] - 1):
        if np.array_equal(maps[c + 1][maps[c]], maps[c][maps[c + 1]]):
            continue
        swapped = maps.copy()
        swapped[[c, c + 1]] = swapped[[c + 1, c]]
        bad = sx.chain_from_maps(pi, a, seed, T, swapped)
        if not np.array_equal(bad, z):
            assert not sx.chain_is_the_recursion(bad, pi, a, seed)
            seen += 1
        if seen == 3:
            break
    assert seen >= 1
