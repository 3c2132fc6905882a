"""The validate-and-reduce passes of include/expfam.h on the MI355X, at the smallest shapes at which they can go wrong, and
the five scalar conjugate models through them against the reference's fixtures.

Tolerances.  Counts and integer sums are exact.  A binary64 sum of positive terms (exponential ``sum``, poisson
``sum_lgamma``, normal ``m2``) is held to 32 eps relative against a long-double NumPy evaluation: both sides add the same
binary64 terms in a different order, and 32 eps is the fixtures' allowance for that.  The normal ``mean`` is held to
32 eps of mean|x| (it is a sum of terms of both signs divided by n).  The split test merges the blocks of two parts on the
host and holds the result to the same 32 eps on a well-conditioned sample (3 + 2 randn).  One ADDITIONAL case, 1e8 + randn,
carries a derived allowance and is marked as such where it is made: there the two means enter the merge formula rounded to
binary64 (half an ulp of 1e8 each) and the formula is first order in that rounding, so a host merge in binary64 cannot do
better than 32 eps + 2 |d| (na nb / n) eps |mean| / m2, with d the difference of the two means.
"""
import numpy as np
import pytest
import torch

import expfam_oracle as orc
from conftest import load_golden

from bayesml_amd import _expfam as xf
from bayesml_amd import bernoulli, categorical, exponential, normal, poisson
from bayesml_amd._exceptions import DataFormatError

pytestmark = pytest.mark.gpu

MODS = {"bernoulli": bernoulli, "categorical": categorical, "poisson": poisson, "exponential": exponential, "normal": normal}
LD = np.longdouble
EPS = orc.EPS
TOL = 32 * EPS
N_GRID = (1, 2, 3, 63, 64, 65, 255, 257, 4097, 100003)
INT_DTYPES = (torch.uint8, torch.int32, torch.int64)
FLT_DTYPES = (torch.float32, torch.float64)
DEGREES = (1, 2, 3, 5, 8, 9, 16, 17, 65, 1000, xf.MAX_DEGREE)          # 8 | 9: registers | LDS bins


@pytest.fixture(scope="module")
def eng():
    return xf.ExpfamPass("cuda:0")


def dev(a, dtype, offset=0):
    """The array on the GPU as a view that starts ``offset`` elements into a larger tensor: a misaligned head for the
    16-byte loads."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    buf = torch.empty(t.numel() + 8, dtype=dtype, device="cuda:0")
    view = buf[offset:offset + t.numel()]
    view.copy_(t.reshape(-1))
    return view


def run(eng, family, x, degree=0):
    return xf.decode(family, eng.stats(family, x, degree))


def close(got, want, scale=None, tol=TOL):
    want = LD(want)
    return abs(LD(got) - want) <= tol * (abs(want) if scale is None else LD(scale))


def int_sample(rng, n, kind):
    if kind == "bernoulli":
        return (rng.random(n) < 0.3).astype(np.int64)
    return rng.poisson(6.0, n).astype(np.int64)


# ---- the N grid x dtype x alignment ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_integer_families_over_sizes_and_alignments(eng, dtype):
    from scipy.special import gammaln
    rng = np.random.default_rng(1)
    for n in N_GRID:
        b, p = int_sample(rng, n, "bernoulli"), int_sample(rng, n, "poisson")
        for off in (0, 1, 3):
            st = run(eng, xf.BERNOULLI, dev(b, dtype, off))
            assert st == dict(n=n, bad=0, n1=int(b.sum()), n0=int(n - b.sum())), (n, off)
            st = run(eng, xf.POISSON, dev(p, dtype, off))
            assert (st["n"], st["bad"], int(st["sum"])) == (n, 0, int(p.sum())), (n, off)
            lg = gammaln(p + 1.0).astype(LD).sum()              # (lgamma is zero at 1 and 2: absolute below a sum of 1)
            assert close(st["sum_lgamma"], lg, scale=max(1.0, float(lg))), (n, off)
            st = run(eng, xf.COUNTS, dev(p % 5, dtype, off), 5)
            assert (st["n"], st["bad"], st["max"]) == (n, 0, int((p % 5).max())), (n, off)
            assert np.array_equal(st["counts"], np.bincount(p % 5, minlength=5)), (n, off)
            st = run(eng, xf.COUNTS, dev(p, dtype, off), 40)
            assert st["bad"] == 0 and np.array_equal(st["counts"], np.bincount(p, minlength=40)), (n, off)


@pytest.mark.parametrize("dtype", FLT_DTYPES)
def test_float_families_over_sizes_and_alignments(eng, dtype):
    rng = np.random.default_rng(2)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for n in N_GRID:
        e = rng.exponential(2.0, n).astype(npdt) + npdt(1e-3)
        g = (3.0 + 2.0 * rng.standard_normal(n)).astype(npdt)
        for off in (0, 1, 3):
            st = run(eng, xf.EXPONENTIAL, dev(e, dtype, off))
            assert (st["n"], st["bad"]) == (n, 0) and close(st["sum"], e.astype(LD).sum()), (n, off)
            st = run(eng, xf.NORMAL, dev(g, dtype, off))
            gl = g.astype(LD)
            mean = gl.sum() / n
            assert st["n"] == n and close(st["mean"], mean, scale=np.abs(gl).mean()), (n, off)
            m2 = ((gl - mean) ** 2).sum()
            assert (st["m2"] == 0.0) if n == 1 else close(st["m2"], m2), (n, off, st["m2"], float(m2))


# ---- determinism and additivity --------------------------------------------------------------------------------------
def _family_inputs():
    rng = np.random.default_rng(3)
    n = 100003
    p = rng.poisson(6.0, n)
    oh = np.zeros((4097, 17), dtype=np.int64)
    oh[np.arange(4097), rng.integers(0, 17, 4097)] = 1
    return [(xf.BERNOULLI, (rng.random(n) < 0.3).astype(np.int64), torch.uint8, 0),
            (xf.COUNTS, p % 7, torch.int32, 7), (xf.COUNTS, p, torch.int64, 64), (xf.ONEHOT, oh, torch.uint8, 17),
            (xf.POISSON, p, torch.int32, 0), (xf.EXPONENTIAL, rng.exponential(1.0, n) + 1e-9, torch.float32, 0),
            (xf.NORMAL, 3.0 + 2.0 * rng.standard_normal(n), torch.float64, 0)]


def _dev2(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to("cuda:0")


def test_two_runs_give_the_same_bits(eng):
    for family, a, dtype, degree in _family_inputs():
        x = _dev2(a, dtype)
        assert torch.equal(eng.stats(family, x, degree), eng.stats(family, x, degree)), family


def test_statistics_of_two_halves_combine_to_the_whole(eng):
    for family, a, dtype, degree in _family_inputs():
        x = _dev2(a, dtype)
        cut = 1 + x.shape[0] // 3
        w, h1, h2 = (run(eng, family, t, degree) for t in (x, x[:cut], x[cut:]))
        assert h1["n"] + h2["n"] == w["n"]
        if family == xf.NORMAL:
            m = orc.merge_normal(h1, h2)
            assert close(m["mean"], w["mean"]) and close(m["m2"], w["m2"]), (m, w)
            continue
        for k in w:
            if k in ("sum_lgamma",) or (family == xf.EXPONENTIAL and k == "sum"):
                assert close(h1[k] + h2[k], w[k]), (family, k)
            elif k == "max":
                assert max(h1[k], h2[k]) == w[k]
            elif k != "n":
                assert np.array_equal(h1[k] + h2[k], w[k]), (family, k)


def test_normal_split_at_1e8_with_the_derived_allowance(eng):
    """An additional case beside the split test above, NOT held to the plain rule: see the module docstring."""
    x = _dev2(1e8 + np.random.default_rng(8).standard_normal(100003), torch.float64)
    cut = 1 + x.shape[0] // 3
    w, h1, h2 = (run(eng, xf.NORMAL, t) for t in (x, x[:cut], x[cut:]))
    m = orc.merge_normal(h1, h2)
    d = h2["mean"] - h1["mean"]
    first_order = 2 * abs(d) * (h1["n"] * h2["n"] / w["n"]) * EPS * abs(w["mean"]) / w["m2"]
    assert close(m["mean"], w["mean"]) and close(m["m2"], w["m2"], tol=TOL + first_order), (m, w, first_order)


def test_integer_sums_are_exact_past_2_to_the_53(eng):
    v = np.full(5000, 2 ** 41 + 1, dtype=np.int64)
    v[::7] = 3
    st = run(eng, xf.POISSON, _dev2(v, torch.int64))
    assert int(v.sum()) > 2 ** 53 and int(st["sum"]) == int(v.sum()) and st["bad"] == 0


# ---- bad values --------------------------------------------------------------------------------------------------------
def _positions(n):
    return [[0], [n - 1], [n // 2], [0, 1, n // 2, n - 2, n - 1]]


@pytest.mark.parametrize("n", (5, 257, 4097))
def test_bad_values_are_counted_left_out_and_refused(eng, n):
    rng = np.random.default_rng(4)
    base = rng.poisson(2.0, n).astype(np.int64) % 2
    cnt = rng.integers(0, 9, n)
    pos = rng.exponential(1.0, n) + 0.5
    for where in _positions(n):
        b = base.copy()
        b[where] = [2, -1, 7, 255, 3][:len(where)]
        st = run(eng, xf.BERNOULLI, _dev2(b, torch.int64))
        keep = np.delete(base, where)
        assert st == dict(n=n, bad=len(where), n1=int(keep.sum()), n0=int(len(keep) - keep.sum()))
        m = bernoulli.LearnModel(device="cuda:0")
        with pytest.raises(DataFormatError):
            m.update_posterior(b)
        assert m.get_hn_params() == dict(hn_alpha=0.5, hn_beta=0.5)

        c = cnt.copy()
        c[where] = [-1, 9, -7, 9, 2 ** 40][:len(where)]           # an index of degree (9) and negative ones: counted, not used
        st = run(eng, xf.COUNTS, _dev2(c, torch.int64), 9)
        assert st["bad"] == len(where) and st["max"] == int(c.max())
        assert np.array_equal(st["counts"], np.bincount(np.delete(cnt, where), minlength=9))
        m = categorical.LearnModel(9, device="cuda:0")
        with pytest.raises(DataFormatError):
            m.update_posterior(c, onehot=False)
        assert np.array_equal(m.hn_alpha_vec, np.full(9, 0.5))

        q = cnt.copy()
        q[where] = -1 - np.arange(len(where))
        st = run(eng, xf.POISSON, _dev2(q, torch.int64))
        assert (st["bad"], int(st["sum"])) == (len(where), int(np.delete(cnt, where).sum()))
        m = poisson.LearnModel(device="cuda:0")
        with pytest.raises(DataFormatError):
            m.update_posterior(q)
        assert (m.hn_alpha, m.hn_beta, m._sum_log_factorial) == (1.0, 1.0, 0.0)

        e = pos.copy()
        e[where] = [np.nan, -0.0, 0.0, -3.0, -np.inf][:len(where)]         # NaN and -0.0 are both outside x > 0
        for dtype in FLT_DTYPES:
            st = run(eng, xf.EXPONENTIAL, _dev2(e, dtype))
            good = np.delete(pos, where).astype(np.float32 if dtype == torch.float32 else np.float64)
            assert st["bad"] == len(where) and close(st["sum"], good.astype(LD).sum())
        m = exponential.LearnModel(device="cuda:0")
        with pytest.raises(DataFormatError):
            m.update_posterior(e)
        assert (m.hn_alpha, m.hn_beta) == (1.0, 1.0)


def test_bad_onehot_rows(eng):
    rng = np.random.default_rng(5)
    n, d = 257, 5
    idx = rng.integers(0, d, n)
    good = np.zeros((n, d), dtype=np.int64)
    good[np.arange(n), idx] = 1
    rows = {0: [0, 0, 0, 0, 0], n // 2: [1, 1, 0, 0, 0], n - 1: [2, -1, 0, 0, 0], 7: [0, 0, 2, 0, 0], 8: [0, -1, 1, 1, 0]}
    for take in ([0], [n - 1], [n // 2], list(rows)):
        x = good.copy()
        for r in take:
            x[r] = rows[r]
        st = run(eng, xf.ONEHOT, _dev2(x, torch.int64), d)
        assert st["bad"] == len(take)
        assert np.array_equal(st["counts"], np.delete(good, take, axis=0).sum(axis=0))
        m = categorical.LearnModel(d, device="cuda:0")
        with pytest.raises(DataFormatError):
            m.update_posterior(x)
        assert np.array_equal(m.hn_alpha_vec, np.full(d, 0.5))


# ---- categorical shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", DEGREES)
def test_onehot_shapes(eng, degree):
    rng = np.random.default_rng(degree)
    n = 263 if degree < 1000 else 70
    idx = rng.integers(0, degree, n)
    idx[:3] = [0, degree - 1, degree // 2]
    cols = torch.from_numpy(idx).to("cuda:0")
    for dtype in INT_DTYPES:
        for pad in (0, 3):
            for off in (0, 1, 3):
                ld = degree + pad
                buf = torch.full((n * ld + 8,), 9, dtype=dtype, device="cuda:0")       # 9 before, between and after the rows:
                x = buf[off:off + n * ld].view(n, ld)[:, :degree]                      # read with the rows' blocks, masked out
                x.zero_()
                x[torch.arange(n, device="cuda:0"), cols] = 1
                xa = eng.adopt(x, "i", cols=degree)
                assert xa.data_ptr() == buf.data_ptr() + off * buf.element_size() and (n == 1 or xa.stride(0) == ld)
                st = run(eng, xf.ONEHOT, xa, degree)
                assert (st["n"], st["bad"]) == (n, 0), (degree, dtype, pad, off)
                assert np.array_equal(st["counts"], np.bincount(idx, minlength=degree)), (degree, dtype, pad, off)
    one = torch.zeros((1, degree), dtype=torch.int64, device="cuda:0")
    one[0, degree - 1] = 1
    st = run(eng, xf.ONEHOT, one, degree)
    assert (st["n"], st["bad"], int(st["counts"][degree - 1]), int(st["counts"].sum())) == (1, 0, 1, 1)


@pytest.mark.parametrize("degree", DEGREES)
def test_index_shapes(eng, degree):
    rng = np.random.default_rng(degree)
    n = 4097
    for dtype in (torch.int32, torch.int64) + ((torch.uint8,) if degree <= 256 else ()):
        for a in (np.zeros(n, dtype=np.int64), np.full(n, degree - 1), rng.integers(0, degree, n)):
            st = run(eng, xf.COUNTS, dev(a, dtype, 1), degree)
            assert (st["n"], st["bad"], st["max"]) == (n, 0, int(a.max()))
            assert np.array_equal(st["counts"], np.bincount(a, minlength=degree)), (degree, dtype)


# ---- normal ------------------------------------------------------------------------------------------------------------
def test_normal_constant_sample_and_single_value(eng):
    for v, dtype in ((0.1, torch.float64), (1e8 + 1.0, torch.float64), (3.3, torch.float32)):
        for n in (1, 3, 257, 100003):
            x = torch.full((n,), v, dtype=dtype, device="cuda:0")
            st = run(eng, xf.NORMAL, x)
            assert st["n"] == n and st["m2"] == 0.0 and st["mean"] == float(x[0]), (v, n, st)


@pytest.mark.parametrize("name", sorted(n for n in orc.CASES if orc.CASES[n][0] == "normal" and orc.CASES[n][4]))
def test_normal_fixture_samples(eng, name):
    for recipe in orc.CASES[name][4]:
        a = orc.make(recipe)
        al = a.astype(LD)
        mean = al.sum() / a.size
        st = run(eng, xf.NORMAL, _dev2(a, torch.float32 if a.dtype == np.float32 else torch.float64))
        assert close(st["mean"], mean) and close(st["m2"], ((al - mean) ** 2).sum()), (name, st)


# ---- the models through the real engine ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(orc.CASES))
def test_fixture_through_the_engine(name):
    fx = load_golden(name + ".npz")

    def prepare(m):
        m._device = "cuda:0"
    got = orc.drive(MODS[orc.CASES[name][0]], name, orc.batches(name, fx), prepare=prepare)
    orc.compare(name, got, fx)


def test_device_tensor_is_used_in_place_and_matches_numpy():
    rng = np.random.default_rng(6)
    a = rng.poisson(3.0, 50000)
    t = torch.from_numpy(a).to("cuda:0")
    m1 = poisson.LearnModel(device="cuda:0").update_posterior(t)
    m2 = poisson.LearnModel(device="cuda:0").update_posterior(a)
    assert m1.get_hn_params() == m2.get_hn_params() and m1._sum_log_factorial == m2._sum_log_factorial
    assert m1.hn_alpha == 1.0 + a.sum() and m1.hn_beta == 1.0 + a.size and m1._engine.launch_info == "expfam_stats_poisson"


# ---- one larger shape per family -------------------------------------------------------------------------------------
def test_larger_shapes_against_torch_reductions(eng):
    """2e7 values made on the device.  Counts and integer sums against torch's int64 reductions on the device; the binary64
    sums against a long-double evaluation of the same values on the host, at the 32 eps of every other sum."""
    n = 20_000_000
    g = torch.Generator(device="cuda:0").manual_seed(7)
    u = torch.rand(n, generator=g, device="cuda:0")
    b = (u < 0.25).to(torch.uint8)
    st = run(eng, xf.BERNOULLI, b)
    assert st == dict(n=n, bad=0, n1=int(b.sum(dtype=torch.int64)), n0=int((b == 0).sum(dtype=torch.int64)))
    idx = (u * 1000).to(torch.int32).clamp_(max=999)
    st = run(eng, xf.COUNTS, idx, 1000)
    assert st["bad"] == 0 and np.array_equal(st["counts"], torch.bincount(idx.to(torch.int64), minlength=1000).cpu().numpy())
    idx8 = (u * 6).to(torch.uint8).clamp_(max=5)
    st = run(eng, xf.COUNTS, idx8, 6)
    assert st["bad"] == 0 and np.array_equal(st["counts"], torch.bincount(idx8.to(torch.int64), minlength=6).cpu().numpy())
    rows = n // 16
    oh = torch.zeros((rows, 16), dtype=torch.uint8, device="cuda:0")
    col = (u[:rows] * 16).to(torch.int64).clamp_(max=15)
    oh[torch.arange(rows, device="cuda:0"), col] = 1
    st = run(eng, xf.ONEHOT, oh, 16)
    assert st["bad"] == 0 and np.array_equal(st["counts"], torch.bincount(col, minlength=16).cpu().numpy())
    k = (-8.0 * torch.log1p(-u)).to(torch.int32)                 # counts with a long tail
    st = run(eng, xf.POISSON, k)
    assert st["bad"] == 0 and int(st["sum"]) == int(k.sum(dtype=torch.int64))
    from scipy.special import gammaln
    vals, cnts = np.unique(k.cpu().numpy(), return_counts=True)
    assert close(st["sum_lgamma"], (gammaln(vals + 1.0).astype(LD) * cnts).sum())
    e = (-torch.log1p(-u)).to(torch.float32) + 1e-6
    st = run(eng, xf.EXPONENTIAL, e)
    assert st["bad"] == 0 and close(st["sum"], e.cpu().numpy().astype(LD).sum())
    x = 1e4 + 0.01 * torch.randn(n, generator=g, device="cuda:0", dtype=torch.float64)
    st = run(eng, xf.NORMAL, x)
    xl = x.cpu().numpy().astype(LD)
    mean = xl.sum() / n
    assert close(st["mean"], mean) and close(st["m2"], ((xl - mean) ** 2).sum())
