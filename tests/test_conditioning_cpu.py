"""What makes the bars of tests/test_gpu_conditioning.py credible, on the CPU: on far-apart, tight, offset, badly scaled
and flat clusters (tests/conditioning_cases.py) the oracle's two-pass statistics stay at rounding level, the engine's
raw-moment formulation loses ``~eps R^2`` of S (and no more), and the kernel-level bar
``max(100 e_emul, 100 e_ref, 1e-12)`` rejects an f32 accumulator and moments about the origin."""
import numpy as np
import pytest

import conditioning_cases as cc

EPS = np.finfo(np.float64).eps


def _case(recipe, R, dtype, **kw):
    c = cc.make(recipe, R, dtype, **kw)
    r = cc.responsibilities(c)
    ref = cc.reference_stats(c.x, r)
    return c, r, ref


@pytest.mark.parametrize("recipe,R,dtype", cc.grid())
def test_oracle_two_pass_stays_at_rounding_level(recipe, R, dtype):
    c, r, ref = _case(recipe, R, dtype)
    e_ref = cc.stat_errors(cc.oracle_stats(c.x, r), ref)
    for key, e in e_ref.items():
        assert e.max() < 1e3 * EPS, (key, e)            # (sums of 20 000 rows)


@pytest.mark.parametrize("recipe,dtype", [(rc, dt) for rc in cc.RECIPES for dt in (np.float32, np.float64)])
def test_raw_moment_loss_grows_as_R_squared(recipe, dtype):
    """e_emul(S) ~ eps (Delta/sigma)^2: measured 0.3 .. 150 eps R^2 (far, sorted, offset, flat; the overlapping pairs of
    ``scales`` lose less).  Bounded above (the model holds, nothing grows faster) and, where R^2 eps dominates rounding,
    growing with R."""
    e = {}
    for R in cc.GRID[dtype]:
        c, r, ref = _case(recipe, R, dtype)
        e_emul = cc.formulation_error(c.x, r, c.pivot, ref)
        e[R] = float(e_emul["s"].max())
        assert e_emul["ns"].max() < 1e3 * EPS and e_emul["x_bar"].max() < 1e3 * EPS, R
        assert e[R] < 500 * EPS * R * R + 1e-12, (R, e[R])
    lo, hi = min(e), max(e)
    assert e[hi] > 1e3 * e[lo], e
    if recipe != "scales":
        assert e[hi] > 0.1 * EPS * hi * hi, e


@pytest.mark.parametrize("recipe,R,dtype", cc.grid())
def test_f32_accumulation_fails_the_bar(recipe, R, dtype):
    c, r, ref = _case(recipe, R, dtype)
    bar = cc.kernel_bar(cc.formulation_error(c.x, r, c.pivot, ref), cc.stat_errors(cc.oracle_stats(c.x, r), ref))
    bad = cc.stat_errors(cc.emulate_engine(c.x, r, c.pivot, acc=np.float32), ref)
    assert np.any(bad["s"] > bar["s"]), (bad["s"], bar["s"])


@pytest.mark.parametrize("R,dtype", [(R, dt) for dt in (np.float32, np.float64) for R in cc.GRID[dt]])
def test_moments_about_the_origin_fail_the_bar_on_offset_rows(R, dtype):
    c, r, ref = _case("offset", R, dtype)
    bar = cc.kernel_bar(cc.formulation_error(c.x, r, c.pivot, ref), cc.stat_errors(cc.oracle_stats(c.x, r), ref))
    bad = cc.stat_errors(cc.emulate_engine(c.x, r, c.pivot, origin=True), ref)
    assert np.any(bad["s"] > bar["s"]), (bad["s"], bar["s"])


@pytest.mark.parametrize("recipe,R,dtype", cc.grid(recipes=("far", "sorted", "offset", "flat")))
def test_bar_admits_other_summation_orders(recipe, R, dtype):
    """The kernels do not sum in the emulation's order: 16-row blocks over the reversed rows stay inside the bar."""
    c, r, ref = _case(recipe, R, dtype)
    bar = cc.kernel_bar(cc.formulation_error(c.x, r, c.pivot, ref), cc.stat_errors(cc.oracle_stats(c.x, r), ref))
    other = cc.stat_errors(cc.emulate_engine(c.x[::-1], r[::-1], c.pivot, block=16), ref)
    for key in other:
        assert np.all(other[key] <= bar[key]), (key, other[key], bar[key])


def test_recipes_are_what_they_claim():
    c = cc.make("sorted", 1e3, np.float64)
    assert np.all(np.diff(c.z) >= 0) and np.sum(c.z == 0) > cc.PIVOT_ROWS      # pivot inside the first cluster
    far = cc.make("far", 1e3, np.float64)
    assert np.array_equal(np.sort(far.x, axis=0), np.sort(c.x, axis=0))
    r = cc.responsibilities(far)
    assert np.all(r.max(axis=1) == 1.0)                                        # far apart: one-hot
    s = cc.make("scales", 1e4, np.float32)
    sd = s.x.astype(np.float64).std(axis=0)
    assert sd.max() / sd.min() > 1e3
    rs = cc.responsibilities(s)
    assert np.mean(rs.max(axis=1) < 0.99) > 0.1                               # the overlapping pairs: soft
    f = cc.make("flat", 1e2, np.float32, D=8)
    assert np.all(f.x[:, -1] == f.x[0, -1]) and np.array_equal(f.x[:, 0], f.z.astype(np.float32))
    o = cc.make("offset", 1e4, np.float32)
    assert np.abs(o.x - cc.OFFSET[np.float32]).max() * 30 < 1.5 * cc.OFFSET[np.float32]
    # the per-component metric: a tight component's error is not hidden by a broad one
    ref = np.array([[1e6, 0.0], [1e-6, 0.0]])
    q = ref + np.array([[0.0, 0.0], [1e-9, 0.0]])
    assert np.allclose(cc.per_component(q, ref), [0.0, 1e-3])
