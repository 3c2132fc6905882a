"""The device samplers (csrc/sample.hip) against the exact oracle of tests/sampler_exact.py at their tile, class-run,
dispatch and chain edges.  Emissions are held to 2 B_j (the bound derived in sampler_exact's docstring), each device normal
to 2 c_e u |e|, float32 output to the bits of the rounded float64 output, class indices and chains to equality; the chains
are ones whose chunk maps do not coalesce, so the state carried across chunk, group and 256-group borders decides z (and,
for the state carried from group to group, ones whose maps of a whole group do not coalesce either).
Every test prints its worst |error| / B_j; profiles/sampler_tests.md records them.  The cases are tests/sampler_cases.py's,
which tests/test_sampler_edges.py checks on the CPU.
"""
import functools

import numpy as np
import pytest
import torch

import sampler_cases as sc
import sampler_exact as sx
from bayesml_amd import _engine, _sample
from oracle import sampler_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMIT = {c.name: c for c in sc.emission_cases()}
GUARD = -7777.25            # exact in float32; no sample equals it
Z_GUARD = -99


def _z(c):
    return torch.as_tensor(np.asarray(c.z, dtype=np.int64), device=DEV)


def _draw(c, dtype=torch.float64, grouped=True):
    return _sample.draw_emissions(_z(c), c.mu, None, c.seed, dtype, row0=c.row0, grouped=grouped, factors=c.a)


@functools.lru_cache(maxsize=None)
def _exact(name):
    c = EMIT[name]
    return sx.Emissions(c.z, c.mu, c.a, c.seed, c.row0)


def _hold(c, grouped):
    ex = _exact(c.name)
    x = _draw(c, grouped=grouped)
    assert x.shape == (len(c.z), c.D) and x.dtype == torch.float64
    r = ex.ratio(x.cpu().numpy())
    print(f"\n[sampler-edges] {c.name} {'grouped' if grouped else 'plain'}: worst |error| / B_j = {r:.3f} (allowed 2)")
    assert r <= 2.0
    return r


# ---- normals alone -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "plain"])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 7, 8])
def test_normals_alone(D, grouped):
    """factors = I, mu = 0: fma(eps, 1, 0) is exact, so x IS the device's normals."""
    n, seed = 257, 4100 + D
    mu, a = np.zeros((1, D)), np.eye(D)[None]
    worst = 0.0
    for row0 in (0, 3, 2 ** 32 + 1, 2 ** 40 + 3):
        z = torch.zeros(n + 40, dtype=torch.int64, device=DEV)
        long = _sample.draw_emissions(z, mu, None, seed, torch.float64, row0=row0, grouped=grouped, factors=a)
        r = sx.normal_ratio(long[:n].cpu().numpy(), seed, row0)
        worst = max(worst, r)
        assert r <= 2.0, row0
        # the window at row0 + 29 is the same rows of the longer draw, bit for bit
        win = _sample.draw_emissions(z[:n], mu, None, seed, torch.float64, row0=row0 + 29, grouped=grouped, factors=a)
        assert torch.equal(win, long[29:29 + n]), row0
    print(f"\n[sampler-edges] normals D = {D} {'grouped' if grouped else 'plain'}: worst |error| / (c_e u |e|) = {worst:.3f} (allowed 2)")


# ---- emissions against 2 B_j -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "plain"])
@pytest.mark.parametrize("D", sc.DISPATCH_D)
def test_emissions_at_every_dispatch_edge(D, grouped):
    _hold(EMIT[f"dispatch-D{D}"], grouped)


def test_degree_601_is_refused_and_nothing_is_launched():
    D, n = 601, 4
    z = torch.zeros(n, dtype=torch.int64, device=DEV)
    with pytest.raises(_engine.EngineError, match="GMMVB_EUNSUPPORTED.*D <= 600"):
        _sample.draw_emissions(z, np.zeros((1, D)), None, 1, torch.float64, factors=np.eye(D)[None])
    lib = _engine.load_library()
    x = torch.full((n, D), GUARD, dtype=torch.float64, device=DEV)
    mu, a = torch.zeros(1, D, dtype=torch.float64, device=DEV), torch.eye(D, dtype=torch.float64, device=DEV)[None].contiguous()
    rc = lib.gmmvb_sample_emissions(1, D, z.data_ptr(), mu.data_ptr(), a.data_ptr(), 1, 0, n, _engine.GMMVB_F64, x.data_ptr(), D,
                                    None, 0, None)
    torch.cuda.synchronize()
    assert rc == 2 and bool((x == GUARD).all())                  # GMMVB_EUNSUPPORTED


@pytest.mark.parametrize("D", [128, 129])
def test_default_factor_path(D):
    """Without ``factors=`` the library factors Lambda itself up to D = 128 and the host does above; the oracle takes the
    factors read back, so their own error stays out."""
    K, n, seed = 3, 70, 4300 + D
    mu, lam = sc.spd_model(K, D, 0)
    z = np.random.default_rng(D).integers(0, K, n)
    if D <= _engine.MAX_MFMA_DEGREE:
        a = _engine.kside_factor(torch.as_tensor(lam, device=DEV))[1].cpu().numpy()
    else:
        a = _sample.emission_factors(lam)
    ex = sx.Emissions(z, mu, a, seed)
    for grouped in (True, False):
        x = _sample.draw_emissions(torch.as_tensor(z, device=DEV), mu, lam, seed, torch.float64, grouped=grouped)
        r = ex.ratio(x.cpu().numpy())
        print(f"\n[sampler-edges] default factors D = {D} {'grouped' if grouped else 'plain'}: worst |error| / B_j = {r:.3f} (allowed 2)")
        assert r <= 2.0
    # the factors are factors of Lambda (loosely: tests/test_gpu_kside*.py hold them to their own bound)
    cov = np.einsum("kij,kil->kjl", np.tril(a), np.tril(a))
    assert np.max(np.abs(cov @ lam - np.eye(D))) < 1e-8


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "plain"])
@pytest.mark.parametrize("name", [c.name for c in sc.class_runs()])
def test_row_count_and_class_run_edges(name, grouped):
    _hold(EMIT[name], grouped)


def test_more_than_8192_classes_take_the_plain_kernel():
    c = EMIT["K8193"]
    assert _engine.load_library().gmmvb_sample_emissions_work_bytes(c.K, len(c.z)) == 0
    assert _engine.load_library().gmmvb_sample_emissions_work_bytes(8192, len(c.z)) == (2 * 8192 + len(c.z)) * 4
    _hold(c, True)


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "plain"])
@pytest.mark.parametrize("name", ["scaled", "cov-x1e+08"])
def test_scale_and_conditioning(name, grouped):
    _hold(EMIT[name], grouped)


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "plain"])
@pytest.mark.parametrize("D", [33, 257])
def test_float32_is_the_rounding_of_float64(D, grouped):
    c = EMIT[f"dispatch-D{D}"]
    x64, x32 = _draw(c, torch.float64, grouped), _draw(c, torch.float32, grouped)
    assert x32.dtype == torch.float32 and torch.equal(x32, x64.float())


# ---- nothing past the end (C ABI) --------------------------------------------------------------------------------------

@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "plain"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 33, 70])
def test_emissions_write_nothing_past_the_end(n, dtype, grouped):
    """The output is rows [2, 2 + n) of a guard-filled buffer with ldx = D + 3: padding columns, the rows before and after
    and the classes must keep their guard; the values are those of the dense call."""
    lib = _engine.load_library()
    c = sc.dispatch(17, n=n)
    D, K, ldx = c.D, c.K, c.D + 3
    buf = torch.full((n + 4, ldx), GUARD, dtype=dtype, device=DEV)
    zbuf = torch.full((n + 4,), Z_GUARD, dtype=torch.int64, device=DEV)
    zbuf[2:2 + n] = _z(c)
    mu, a = _sample._up(c.mu, DEV), _sample._up(c.a, DEV)
    nbytes = lib.gmmvb_sample_emissions_work_bytes(K, n) if grouped else 0
    assert nbytes == ((2 * K + n) * 4 if grouped else 0)
    work = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = lib.gmmvb_sample_emissions(K, D, zbuf[2:].data_ptr(), mu.data_ptr(), a.data_ptr(), c.seed, 0, n, _sample._dtype_code(dtype),
                                    buf[2:].data_ptr(), ldx, work.data_ptr() if grouped else None, nbytes, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(buf[2:2 + n, :D], _draw(c, dtype, grouped))
    assert bool((buf[:2] == GUARD).all()) and bool((buf[2 + n:] == GUARD).all()) and bool((buf[:, D:] == GUARD).all())
    assert bool((zbuf[:2] == Z_GUARD).all()) and bool((zbuf[2 + n:] == Z_GUARD).all()) and torch.equal(zbuf[2:2 + n], _z(c))
    assert bool((work[nbytes:] == 0x5A).all())


@pytest.mark.parametrize("rem", [0, 1, 2, 3])
def test_latent_writes_nothing_past_the_end(rem):
    """row0 % 4 = rem: the first and the last block of four rows are cut on either side."""
    lib = _engine.load_library()
    pi = np.array([0.1, 0.2, 0.3, 0.4])
    cdf = _sample._up(np.cumsum(pi), DEV)
    for n in (1, 2, 3, 4, 5):
        row0 = 4 * 1000 + rem
        zbuf = torch.full((n + 8,), Z_GUARD, dtype=torch.int64, device=DEV)
        rc = lib.gmmvb_sample_latent(4, cdf.data_ptr(), 5100, row0, n, zbuf[4:].data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0
        got = zbuf.cpu().numpy()
        assert np.all(got[:4] == Z_GUARD) and np.all(got[4 + n:] == Z_GUARD), (rem, n)
        assert np.array_equal(got[4:4 + n], so.mixture_latent(pi, 5100, row0, n)), (rem, n)


def test_zero_rows_write_nothing():
    lib = _engine.load_library()
    D = 5
    x = torch.full((3, D), GUARD, dtype=torch.float64, device=DEV)
    z = torch.full((3,), Z_GUARD, dtype=torch.int64, device=DEV)
    mu, a, cdf = _sample._up(np.zeros((1, D)), DEV), _sample._up(np.eye(D)[None], DEV), _sample._up(np.ones(1), DEV)
    work = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    assert lib.gmmvb_sample_emissions(1, D, z.data_ptr(), mu.data_ptr(), a.data_ptr(), 1, 0, 0, _engine.GMMVB_F64, x.data_ptr(), D,
                                      work.data_ptr(), 1024, None) == 0
    assert lib.gmmvb_sample_latent(1, cdf.data_ptr(), 1, 7, 0, z.data_ptr(), None) == 0
    assert lib.gmmvb_sample_chain(1, cdf.data_ptr(), cdf.data_ptr(), 1, 0, z.data_ptr(), work.data_ptr(), 1024, None) == 0
    torch.cuda.synchronize()
    assert bool((x == GUARD).all()) and bool((z == Z_GUARD).all()) and bool((work == 0).all())


# ---- latent classes ----------------------------------------------------------------------------------------------------

def _latent(pi, seed, row0, n):
    lib = _engine.load_library()
    z = torch.empty(n, dtype=torch.int64, device=DEV)
    cdf = _sample._up(np.cumsum(pi), DEV)
    _engine._check(lib, lib.gmmvb_sample_latent(len(pi), cdf.data_ptr(), seed, row0, n, z.data_ptr(), None), "gmmvb_sample_latent")
    torch.cuda.synchronize()
    return z


@pytest.mark.parametrize("name", list(sc.latent_pis()))
def test_latent_classes_equal_the_host(name):
    pi = sc.latent_pis()[name]
    for row0, n in ((0, 3001), (2 ** 40 + 3, 3001)):
        z = _latent(pi, 5200, row0, n).cpu().numpy()
        assert np.array_equal(z, so.mixture_latent(pi, 5200, row0, n)), row0
        assert np.all(pi[z] > 0), "a class of probability 0 was drawn"


def test_latent_refuses_more_than_8192_classes():
    with pytest.raises(_engine.EngineError, match="GMMVB_EUNSUPPORTED.*K <= 8192"):
        _latent(np.full(8193, 1.0 / 8193), 1, 0, 10)


def test_latent_grid_stride_loop():
    """n = 2^26 + 1000: more blocks of four rows than 2^16 workgroups of 256 threads cover, so the stride loop runs: its
    second trip starts 2^26 rows after the first block, inside the last window."""
    pi = np.array([0.05, 0.35, 0.0, 0.2, 0.4])
    n, seed, row0 = 2 ** 26 + 1000, 5300, 2
    z = _latent(pi, seed, row0, n)
    assert z.shape == (n,)
    for lo in (0, 2 ** 25 - 2048, n - 4096):                     # the last one runs from row 2^26 - 3096 to the end
        assert np.array_equal(z[lo:lo + 4096].cpu().numpy(), so.mixture_latent(pi, seed, row0 + lo, 4096)), lo
    assert int(z.min()) == 0 and int(z.max()) == 4
    freq = torch.bincount(z, minlength=5).double().cpu().numpy() / n
    assert freq[2] == 0.0 and np.max(np.abs(freq - pi)) < 5 * np.sqrt(0.25 / n)


# ---- chains that do not coalesce ---------------------------------------------------------------------------------------

def _chain_case(name, T, groups=False):
    pi, a = sc.CHAINS[name]()
    seed = sc.chain_seed(name, T)
    maps = sx.chunk_maps(pi, a, seed, T)
    non, of = sx.nonconstant_maps(maps[1:]), maps.shape[0] - 1
    assert 2 * non >= of, "the case's chunk maps coalesce: it would not test the carry"
    if groups:
        gm = sx.group_maps(maps)
        assert 2 * sx.nonconstant_maps(gm[1:]) >= gm.shape[0] - 1, "the case's group maps coalesce"
    z = _sample.markov_chain(pi, a, T, seed, DEV)
    assert z.shape == (T,) and z.dtype == torch.int64
    first = sx.chain_first_mismatch(z.cpu().numpy(), pi, a, seed)
    assert first == -1, f"z[{first}] is not one step of the recursion from z[{first - 1}]"
    assert torch.equal(z, _sample.markov_chain(pi, a, T, seed, DEV))
    return non, of


@pytest.mark.parametrize("T", sc.CHAIN_T)
@pytest.mark.parametrize("name", list(sc.CHAINS))
def test_chain_is_the_recursion(name, T):
    _chain_case(name, T)


@pytest.mark.parametrize("name", sc.LONG_CHAINS)
def test_chain_across_the_256_group_border(name):
    """T = 2^24 + 1029: 257 groups, so the loop that hands every group's chunks their entry states takes a second trip."""
    non, of = _chain_case(name, sc.LONG_T)
    print(f"\n[sampler-edges] {name} T = 2^24 + 1029: {non} of {of} chunk maps after the first are non-constant")


@pytest.mark.parametrize("name,T", [(name, T) for name, Ts in sc.GROUP_CHAINS.items() for T in Ts])
def test_chain_carries_the_state_from_group_to_group(name, T):
    """Chains that do not forget their start within a group of 65536 steps, over four groups and over 257: the state that
    thread 0 of ``chain_starts_kernel`` carries from group to group decides every later z."""
    _chain_case(name, T, groups=True)
