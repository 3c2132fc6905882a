"""Oracles of the scalar conjugate families' prequential pass, include/expseq.h (TEST INFRASTRUCTURE ONLY).

(a) ``restate``: the pass in NumPy with the device's fixed tree (csrc/expseq_kernels.h; the tile and scan constants are
    imported from ``bayesml_amd._expseq``), every operation rounded on its own as on the device.  ``CpuSequencePass`` wraps
    it as a stand-in for ``_expseq.SequencePass`` behind the private ``LearnModel._expseq_pass_factory`` seam.
(b) ``Exact``: the reference's recursion in exact arithmetic.  Every binary64 value is a dyadic rational, so the prefix
    statistics are sums of Python integers at a common scale and the parameters are ``fractions.Fraction``; the code
    lengths are mpmath at 50 digits (``nats_mp``, which also returns the sum of the magnitudes of the formula's terms).
(c) ``loop``: the per-value loop over the package's own ``pred_and_update`` (host only).
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import torch

from bayesml_amd import _expfam as xf
from bayesml_amd import _expseq as xs

mp.mp.dps = 50
EPS = 2.0 ** -52
T, W, ITEMS, THREADS = xs.TILE, xs.SCAN_THREADS, xs.ITEMS, xs.THREADS
LANES = 64
EDGE_LENGTHS = (1, 2, T - 1, T, T + 1, 3 * T + 17, W * T + 3 * T + 17)


# ---- (a) the fixed tree ---------------------------------------------------------------------------------------------------
class AddOp:
    """Component-wise addition (integer counts and sums, binary64 sums)."""

    def __init__(self, dtypes):
        self.dtypes = dtypes

    def identity(self, shape):
        return tuple(np.zeros(shape, dtype=d) for d in self.dtypes)

    @staticmethod
    def combine(a, b):
        return tuple(u + v for u, v in zip(a, b))


class MergeOp:
    """The (n, mean, m2) merge of include/expfam.h, earlier block on the left."""
    dtypes = (np.float64,) * 3

    def identity(self, shape):
        return tuple(np.zeros(shape) for _ in range(3))

    @staticmethod
    def combine(a, b):
        a, b = np.broadcast_arrays(*a), np.broadcast_arrays(*b)
        (na, ma, sa), (nb, mb, sb) = a, b
        with np.errstate(invalid="ignore", divide="ignore"):
            n = na + nb
            d = mb - ma
            r = nb / n
            mean = ma + d * r
            m2 = sa + sb + d * d * na * r
        ea, eb = nb == 0.0, (na == 0.0) & (nb != 0.0)
        return tuple(np.where(ea, u, np.where(eb, v, w)) for u, v, w in zip(a, b, (n, mean, m2)))


def _shift(op, s, off):
    """Every lane's value from `off` lanes earlier; the identity where there is none."""
    return tuple(np.concatenate([i, c[..., :-off]], axis=-1) for c, i in zip(s, op.identity(s[0].shape[:-1] + (off,))))


def block_scan(op, t):
    """csrc/expseq_kernels.h: block_scan over thread totals [G, 256] -> (what lies before each thread, the totals [G])."""
    g = t[0].shape[0]
    inc = tuple(c.reshape(g, THREADS // LANES, LANES) for c in t)
    off = 1
    while off < LANES:
        inc = op.combine(_shift(op, inc, off), inc)
        off <<= 1
    exc = _shift(op, inc, 1)
    tot, bases = op.identity((g,)), []
    for w in range(THREADS // LANES):
        bases.append(tot)
        tot = op.combine(tot, tuple(c[:, w, LANES - 1] for c in inc))
    base = tuple(np.stack([b[k] for b in bases], axis=1)[:, :, None] for k in range(len(tot)))
    before = op.combine(base, exc)
    return tuple(np.ascontiguousarray(np.broadcast_to(c, exc[0].shape)).reshape(g, THREADS) for c in before), tot


def _fold_last_axis(op, s):
    t = op.identity(s[0].shape[:-1])
    for k in range(s[0].shape[-1]):
        t = op.combine(t, tuple(c[..., k] for c in s))
    return t


def exclusive_prefix(op, items, n):
    """The statistics of positions 0 .. i-1 for every i < n, in the device's order.  ``items`` are the per-position
    statistics (tuple of [n] arrays); positions past n are the identity."""
    tiles = (n + T - 1) // T
    pad = tuple(np.concatenate([c, i]) for c, i in zip(items, op.identity((tiles * T - n,))))
    it = tuple(c.reshape(tiles, THREADS, ITEMS) for c in pad)
    before, agg = block_scan(op, _fold_last_axis(op, it))
    # scan_kernel: thread j owns tiles j * per .. (j + 1) * per - 1
    per = (tiles + W - 1) // W
    ag = tuple(np.concatenate([c, i]).reshape(1, W, per) for c, i in zip(agg, op.identity((W * per - tiles,))))
    run, _ = block_scan(op, _fold_last_axis(op, ag))
    carry = []
    for k in range(per):
        carry.append(run)
        run = op.combine(run, tuple(c[..., k] for c in ag))
    carry = tuple(np.stack([c[j] for c in carry], axis=-1).reshape(-1)[:tiles] for j in range(len(run)))
    run = op.combine(tuple(c[:, None] for c in carry), before)
    out = []
    for k in range(ITEMS):
        out.append(run)
        run = op.combine(run, tuple(c[..., k] for c in it))
    return tuple(np.stack([o[j] for o in out], axis=-1).reshape(-1)[:n] for j in range(len(run)))


def longest_path(n):
    """A of the derived bounds: the additions / merges on the longest path of the tree to one position, plus one.  Items of
    a thread (ITEMS - 1 to its total, ITEMS - 1 more onto its base), six Hillis-Steele steps and THREADS / 64 wave totals
    in the tile and again in the scan workgroup, the scan thread's own tiles twice (its total, then the walk), the carry
    onto the thread's base, and the start value."""
    tiles = (n + T - 1) // T
    per = (tiles + W - 1) // W
    block = 6 + THREADS // LANES + 1
    return 2 * (ITEMS - 1) + block + 2 * (per - 1) + block + 1 + 1 + 1


def restate(family, x, start, nats=True):
    """(parameter arrays in the order of ``_expseq.PARAMS``, nats, bad count) of the sample x (ndarray in its storage dtype)
    from ``start``: what the device pass returns."""
    from scipy.special import gammaln
    n = x.shape[0]
    i = np.arange(n, dtype=np.float64)
    code = None
    with np.errstate(invalid="ignore", divide="ignore"):
        if family == xs.BERNOULLI:
            one, zero = x == 1, x == 0
            c1, c0, bad = exclusive_prefix(AddOp((np.int64,) * 3), (one.astype(np.int64), zero.astype(np.int64),
                                                                    (~one & ~zero).astype(np.int64)), n)
            a, b = start[0] + c1.astype(np.float64), start[1] + c0.astype(np.float64)
            params = (a / (a + b),)
            if nats:
                code = np.where(one, -np.log(a / (a + b)), np.where(zero, -np.log(b / (a + b)), np.nan))
            nbad = int((~one & ~zero).sum())
        elif family == xs.POISSON:
            ok = x >= 0
            s, _ = exclusive_prefix(AddOp((np.int64,) * 2), (np.where(ok, x, 0).astype(np.int64), (~ok).astype(np.int64)), n)
            r, beta = start[0] + s.astype(np.float64), start[1] + i
            params = (r, 1.0 / (1.0 + beta))
            if nats:
                xd = x.astype(np.float64)
                code = np.where(ok, -(lgamma_step(r, xd) - gammaln(xd + 1.0) - r * np.log1p(1.0 / beta) - xd * np.log1p(beta)), np.nan)
            nbad = int((~ok).sum())
        elif family == xs.EXPONENTIAL:
            xd = x.astype(np.float64)
            ok = xd > 0
            s, _ = exclusive_prefix(AddOp((np.float64, np.int64)), (np.where(ok, xd, 0.0), (~ok).astype(np.int64)), n)
            kappa, lam = start[0] + i, start[1] + s
            params = (kappa, lam)
            if nats:
                code = np.where(ok, -(np.log(kappa) - np.log(lam + xd) - kappa * np.log1p(xd / lam)), np.nan)
            nbad = int((~ok).sum())
        else:
            xd = x.astype(np.float64)
            pivot = xd[0]
            cnt, mean, m2 = exclusive_prefix(MergeOp(), (np.ones(n), xd - pivot, np.zeros(n)), n)
            m0, k0, a0, b0 = (np.float64(v) for v in start)
            mrel, kn, d = m0 - pivot, k0 + cnt, mean - (m0 - pivot)
            beta = b0 + (m2 + cnt * k0 / kn * (d * d)) / 2.0
            alpha = a0 + cnt * 0.5
            mu = np.where(cnt == 0.0, m0, pivot + (k0 * mrel + cnt * mean) / kn)
            nu, lam = 2.0 * alpha, kn / (kn + 1.0) * alpha / beta
            params = (mu, nu, lam)
            if nats:
                e = xd - mu
                code = lgamma_half_step(alpha) + 0.5 * np.log(np.pi * nu / lam) + (nu + 1.0) / 2.0 * np.log1p(lam * (e * e) / nu)
            nbad = 0
    return params, code, nbad


def _tail(v):
    r = 1.0 / v
    r2 = r * r
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))))


def lgamma_half_step(a):
    from scipy.special import gammaln
    big = np.maximum(a, 64.0)
    return np.where(a < 64.0, gammaln(a) - gammaln(a + 0.5),
                    -(big * np.log1p(0.5 / big) + 0.5 * np.log(big) - 0.5 + (_tail(big + 0.5) - _tail(big))))


def lgamma_step(r, x):
    from scipy.special import gammaln
    big = np.maximum(r, 64.0)
    return np.where(r < 64.0, gammaln(r + x) - gammaln(r),
                    (big - 0.5) * np.log1p(x / big) + x * np.log(big + x) - x + (_tail(big + x) - _tail(big)))


def row_indices(x, degree):
    """A one-hot matrix as indices; -1 for a row with a negative entry or a sum other than 1 (include/expfam.h)."""
    v = x.astype(np.int64)
    good = (v >= 0).all(axis=1) & (v.sum(axis=1) == 1)
    return np.where(good, v.argmax(axis=1), -1)


def restate_categorical(x, onehot, alpha, want=None, nats=True):
    """(rows | argmax | None, nats, final counts, bad) of include/expseq.h's categorical pass.  Integer state: no tree to
    restate, the closed forms are the device's expressions."""
    degree = alpha.shape[0]
    k = row_indices(x, degree) if onehot else x.astype(np.int64)
    n = k.shape[0]
    ok = (k >= 0) & (k < degree)
    kk = np.where(ok, k, 0)
    norm = alpha.sum() + np.arange(n, dtype=np.float64)
    # occurrences of the position's own symbol before it: its rank in a stable sort by symbol, minus the symbol's first rank
    order = np.argsort(np.where(ok, k, degree), kind="stable")
    ranks = np.empty(n, dtype=np.int64)
    ranks[order] = np.arange(n)
    first = np.concatenate([[0], np.cumsum(np.bincount(kk[ok], minlength=degree))])[:-1]
    before = ranks - first[kk]
    code = None
    if nats:
        with np.errstate(invalid="ignore"):
            code = np.where(ok, -np.log((alpha[kk] + before.astype(np.float64)) / norm), np.nan)
    pred = None
    if want is not None:
        hot = np.zeros((n, degree), dtype=np.int64)
        hot[np.arange(n)[ok], k[ok]] = 1
        cum = np.cumsum(hot, axis=0) - hot
        pred = (alpha[None, :] + cum.astype(np.float64)) / norm[:, None]
        if want == "argmax":
            pred = np.argmax(pred, axis=1).astype(np.int64)
    return pred, code, np.bincount(kk[ok], minlength=degree).astype(np.int64), int((~ok).sum())


class CpuSequencePass:
    """Stand-in for ``_expseq.SequencePass``: the restatement on CPU tensors."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.launch_info = "cpu restatement"
        self.calls = []

    def adopt(self, a, kind, cols=None):
        return xf.adopt_tensor(a, self.device, kind, cols)

    def run_categorical(self, x, onehot, alpha, want=None, nats=True, chunk_bytes=None):
        alpha = np.asarray(alpha, dtype=np.float64)
        degree, n = alpha.shape[0], x.shape[0]
        assert xf.code(x.dtype) in (0, 1, 2) and x.dim() == (2 if onehot else 1) and n >= 1
        self.passes = -(-n // min(xs.chunk_len(degree, chunk_bytes), n))
        self.calls.append((xs.CATEGORICAL, x.dtype, n, want, nats))
        pred, code, counts, bad = restate_categorical(x.numpy(), onehot, alpha, want, nats)
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))          # noqa: E731
        return t(pred), t(code), t(counts), torch.tensor([bad], dtype=torch.int64)

    def run(self, family, x, start, params=True, nats=True):
        assert x.dim() == 1 and x.shape[0] >= 1 and xf.code(x.dtype) in ((0, 1, 2) if xs.KIND[family] == "i" else (3, 4))
        assert len(start) == xs.N_START[family]
        self.calls.append((family, x.dtype, x.shape[0], params, nats))
        p, code, bad = restate(family, x.numpy(), [float(v) for v in start], nats)
        return (tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in p) if params else None,
                torch.from_numpy(np.ascontiguousarray(code)) if nats else None, torch.tensor([bad], dtype=torch.int64))

    def close(self):
        pass


def use_cpu(model):
    """Route a LearnModel's statistics pass and its sequence pass through the CPU stand-ins; every ``model._seq_pass()``
    gives the same stand-in, so that a test can read its calls."""
    from fake_expfam_engine import cpu_factory
    model._expfam_pass_factory = cpu_factory
    model._expseq_pass_factory = _Same(CpuSequencePass())
    return model


class _Same:
    """A factory that hands out one object (a class, not a closure: the model must stay picklable)."""

    def __init__(self, eng):
        self.eng = eng

    def __call__(self):
        return self.eng


# ---- (b) exact ----------------------------------------------------------------------------------------------------------------
def _dyadic(v):
    """Binary64 values as Python integers at one common power-of-two scale: (object array of ints, scale exponent e) with
    value = int * 2**e."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))
    mi = (m * 2.0 ** 53).astype(np.int64)
    e = e.astype(np.int64) - 53
    e = np.where(mi == 0, np.int64(2 ** 40), e)
    emin = int(e.min()) if np.any(mi != 0) else 0
    return np.array([int(a) << int(b - emin) if a else 0 for a, b in zip(mi, e)], dtype=object), emin


def _frac(i, e):
    return Fraction(int(i)) * (Fraction(2) ** int(e))


class Exact:
    """Exact parameters of any position.  ``params(i)`` gives Fractions in the order of ``_expseq.PARAMS``."""

    def __init__(self, family, x, start):
        self.family, self.n = family, x.shape[0]
        self.start = [Fraction(float(v)) for v in start]
        zero = np.zeros(1, dtype=object)
        if family == xs.BERNOULLI:
            self.c1 = np.concatenate([[0], np.cumsum(x == 1)])
            self.c0 = np.concatenate([[0], np.cumsum(x == 0)])
        elif family == xs.POISSON:
            self.s = np.concatenate([zero, np.cumsum(x.astype(object))])
        elif family == xs.EXPONENTIAL:
            ints, self.e = _dyadic(x)
            self.s = np.concatenate([zero, np.cumsum(ints)])
        else:
            # about the pivot, which is exact here too: x - pivot as integers at the common scale of x and the pivot
            ints, self.e = _dyadic(x)
            v = ints - ints[0]
            self.pivot = _frac(ints[0], self.e)
            self.s1 = np.concatenate([zero, np.cumsum(v)])
            self.s2 = np.concatenate([zero, np.cumsum(v * v)])

    def params(self, i):
        st = self.start
        if self.family == xs.BERNOULLI:
            a, b = st[0] + int(self.c1[i]), st[1] + int(self.c0[i])
            return (a / (a + b),)
        if self.family == xs.POISSON:
            return (st[0] + int(self.s[i]), 1 / (1 + st[1] + i))
        if self.family == xs.EXPONENTIAL:
            return (st[0] + i, st[1] + _frac(self.s[i], self.e))
        m0, k0, a0, b0 = st
        if i == 0:
            return (m0, 2 * a0, k0 / (k0 + 1) * a0 / b0)
        s1, s2 = _frac(self.s1[i], self.e), _frac(self.s2[i], 2 * self.e)
        mean, m2 = s1 / i, s2 - s1 * s1 / i
        xbar = self.pivot + mean
        beta = b0 + (m2 + i * k0 / (k0 + i) * (xbar - m0) ** 2) / 2
        m, kn, alpha = (k0 * m0 + i * xbar) / (k0 + i), k0 + i, a0 + Fraction(i, 2)
        return (m, 2 * alpha, kn / (kn + 1) * alpha / beta)

    def beta(self, i):
        """hn_beta of the normal family before position i (the quantity the derived bound is stated for)."""
        _, nu, lam = self.params(i)
        kn = self.start[1] + i
        return kn / (kn + 1) * (nu / 2) / lam


def _mpf(v):
    return mp.mpf(v.numerator) / mp.mpf(v.denominator) if isinstance(v, Fraction) else mp.mpf(float(v))


def nats_mp(family, params, x, beta_i=None):
    """(-ln of the predictive density of x at the parameters, B = the sum of the magnitudes of the formula's terms) in
    mpmath.  ``params`` in the order of ``_expseq.PARAMS`` (floats or Fractions); poisson takes beta = hn_beta + i through
    ``beta_i`` (p_theta = 1 / (1 + beta) does not hold it exactly)."""
    x = mp.mpf(int(x)) if isinstance(x, (int, np.integer)) else mp.mpf(float(x))
    if family == xs.BERNOULLI:
        p = _mpf(params[0])
        v = -mp.log(p if x == 1 else 1 - p)
        return v, abs(v)
    if family == xs.POISSON:
        r, b = _mpf(params[0]), _mpf(beta_i)
        terms = [mp.loggamma(x + r), -mp.loggamma(r), -mp.loggamma(x + 1), -r * mp.log1p(1 / b), -x * mp.log1p(b)]
    elif family == xs.EXPONENTIAL:
        k, l = _mpf(params[0]), _mpf(params[1])
        terms = [mp.log(k), -mp.log(l + x), -k * mp.log1p(x / l)]
    else:
        mu, nu, lam = (_mpf(p) for p in params)
        terms = [-mp.loggamma(nu / 2), mp.loggamma((nu + 1) / 2), -mp.log(mp.pi * nu / lam) / 2,
                 -(nu + 1) / 2 * mp.log1p(lam * (x - mu) ** 2 / nu)]
    return -mp.fsum(terms), mp.fsum(abs(t) for t in terms)


def positions(n, extra=64, seed=0):
    """Where the exact oracle is evaluated: both ends, every tile, wave and thread edge within reach, and a seeded draw."""
    edges = [0, 1, 2, ITEMS - 1, ITEMS, ITEMS + 1, LANES * ITEMS - 1, LANES * ITEMS, LANES * ITEMS + 1]
    for t in (1, 2, 3, W, W + 1):
        edges += [t * T - 1, t * T, t * T + 1]
    edges += [n - 2, n - 1]
    draw = np.random.default_rng(seed).integers(0, n, extra)
    return sorted({int(p) for p in list(edges) + list(draw) if 0 <= p < n})


# ---- (c) the loop ---------------------------------------------------------------------------------------------------------------
def loop(model, x, loss, names):
    """``[pred_and_update(x[i], loss)]`` with the parameters before each update and the code lengths
    ``-log(_calc_pred_density(x[i]))``: (predictions, {name: array}, nats)."""
    preds, par, code = [], {k: [] for k in names}, []
    for v in x:
        v = v.item() if isinstance(v, np.generic) else v
        model.calc_pred_dist()
        code.append(-np.log(model._calc_pred_density(v)))
        preds.append(model.pred_and_update(v, loss))
        for k in names:
            par[k].append(getattr(model, k))
    return preds, {k: np.array(v, dtype=np.float64) for k, v in par.items()}, np.array(code, dtype=np.float64)


def sample(family, n, seed=0, dtype=None, recipe=None):
    """Seeded samples of the tests."""
    rng = np.random.default_rng(seed)
    if family == xs.BERNOULLI:
        return rng.integers(0, 2, n).astype(dtype or np.int64)
    if family == xs.POISSON:
        return rng.poisson(3.7, n).astype(dtype or np.int64)
    if family == xs.EXPONENTIAL:
        return (rng.exponential(2.0, n) + 1e-3).astype(dtype or np.float64)
    if recipe == "tight":
        return (1e6 + 1e-2 * rng.standard_normal(n)).astype(dtype or np.float64)
    if recipe == "offset":
        return (1e4 + rng.standard_normal(n)).astype(dtype or np.float64)
    return rng.standard_normal(n).astype(dtype or np.float64)


# ---- the checks that the CPU tests (on the restatement) and the GPU tests (on the device) share -------------------------------
def models():
    from bayesml_amd import bernoulli, exponential, normal, poisson
    return {xs.BERNOULLI: bernoulli, xs.POISSON: poisson, xs.EXPONENTIAL: exponential, xs.NORMAL: normal}


LOSSES = {xs.BERNOULLI: ("squared", "0-1", "abs", "KL"), xs.POISSON: ("squared", "0-1", "abs"),
          xs.EXPONENTIAL: ("squared", "0-1", "abs"), xs.NORMAL: ("squared", "0-1", "abs")}      # the losses that return numbers
HN = {xs.BERNOULLI: ("hn_alpha", "hn_beta"), xs.POISSON: ("hn_alpha", "hn_beta"), xs.EXPONENTIAL: ("hn_alpha", "hn_beta"),
      xs.NORMAL: ("hn_m", "hn_kappa", "hn_alpha", "hn_beta")}
DYADIC = {xs.BERNOULLI: (1.5, 2.5), xs.POISSON: (2.5, 1.5)}
NON_DYADIC = {xs.BERNOULLI: (0.3 + 0.7 * math.sqrt(1), 0.3 + 0.7 * math.sqrt(2)),
              xs.POISSON: (0.3 + 0.7 * math.sqrt(1), 0.3 + 0.7 * math.sqrt(2))}


def model(family, start=None, prepare=None, **kw):
    m = models()[family].LearnModel(**kw)
    if start is not None:
        m.set_hn_params(*start)
    return prepare(m) if prepare is not None else m


def hn_of(m, family):
    return [getattr(m, k) for k in HN[family]]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return np.array_equal(a.astype(np.float64).view(np.int64), b.astype(np.float64).view(np.int64))
    return np.array_equal(a, b)


def engine_params(m, family, x, start):
    """The parameter arrays and nats straight from the model's sequence pass (device or stand-in), as NumPy."""
    eng = m._seq_pass()
    p, code, status = eng.run(family, eng.adopt(x, xs.KIND[family]), start)
    assert int(status.cpu()[0]) == 0
    return tuple(t.cpu().numpy() for t in p), code.cpu().numpy()


def check_integer_state(family, n, prepare, with_loop, **kw):
    """Issue test 2: dyadic start -> bit for bit the loop (or, past ``with_loop``, the one-rounding form on NumPy's exact
    integer prefix sums, which is the loop's value for a dyadic start); non-dyadic start -> bit for bit the restatement and
    within 3 eps of the exact value (the add, the normaliser and the divide)."""
    x = sample(family, n, seed=n)
    start = DYADIC[family]
    names = xs.PARAMS[family]
    params, _ = engine_params(model(family, start, prepare, **kw), family, x, start)
    if with_loop:
        want = None
        for loss in LOSSES[family]:
            if loss == "abs" and family == xs.POISSON and n > 300:
                continue          # (SciPy's median costs a millisecond per value: the short lengths and the 300-value fixtures cover it)
            preds, par, _ = loop(model(family, start), x, loss, names)
            lm = model(family, start)
            for v in x:
                lm.pred_and_update(v.item(), loss)
            m = model(family, start, prepare, **kw)
            got = m.pred_and_update_sequence(x, loss)
            assert same_bits(got, np.array(preds)), (family, n, loss)
            assert hn_of(m, family) == hn_of(lm, family), (family, n, loss)
            assert [getattr(m, k) for k in names] == [par[k][-1] for k in names]
            want = par
        for k, got in zip(names, params):
            assert same_bits(got, want[k]), (family, n, k)
    else:
        i = np.arange(n, dtype=np.float64)
        if family == xs.BERNOULLI:
            c1 = np.concatenate([[0], np.cumsum(x == 1)[:-1]])
            a, b = start[0] + c1, start[1] + (i - c1)
            want = (a / (a + b),)
        else:
            s = np.concatenate([[0], np.cumsum(x.astype(np.int64))[:-1]])
            want = (start[0] + s, 1.0 / (1.0 + (start[1] + i)))
        for k, got, w in zip(names, params, want):
            assert same_bits(got, w), (family, n, k)
        m = model(family, start, prepare, **kw)
        m.pred_and_update_sequence(x)
        up = model(family, start, prepare, **kw).update_posterior(x)
        assert hn_of(m, family) == hn_of(up, family)
    # non-dyadic
    start = NON_DYADIC[family]
    params, _ = engine_params(model(family, start, prepare, **kw), family, x, start)
    ref, _, _ = restate(family, x, start, nats=False)
    ex = Exact(family, x, start)
    for k, got, w in zip(names, params, ref):
        assert same_bits(got, w), (family, n, k)
    for i in positions(n):
        for got, e in zip(params, ex.params(i)):
            assert abs(Fraction(float(got[i])) - e) <= 3 * EPS * abs(e), (family, n, i)


FLOAT_START = {"exp": (1.25, 0.75), "std": (0.0, 1.0, 1.0, 1.0), "tight": (1e6, 1.0, 1.0, 1.0), "offset": (0.0, 1.0, 1.0, 1.0)}


def normal_bounds(x, start, i, a_path, mu, beta):
    """The derived bounds of the normal family at position i (issue test 3).  16 = the roundings of one merge (n, d, r,
    d r, the mean's add; d d, (d d) na, ((d d) na) r and two adds for m2: 10) plus the fold's on the path to beta (m - p,
    d, d d, n k0, / kn, the product, the add, the halving, the final add: 9), rounded down to the issue's figure: the fold's
    roundings happen once, not once per tree level, so 16 per level bounds them with room."""
    xd = x.astype(np.float64)
    p = xd[0]
    r = abs(float(start[0]) - p) + (np.max(np.abs(xd[:i] - p)) if i else 0.0)
    return (16 * a_path * EPS * r + 2 * EPS * abs(float(mu)), 16 * a_path * EPS * (float(start[3]) + i * r * r))


def check_float_state(family, n, dtype, recipe, prepare, **kw):
    """Issue test 3: parameters against the exact oracle under the bounds derived from the tree; kappa and p_nu bit for bit
    the restatement's."""
    x = sample(family, n, seed=n + 1, dtype=dtype, recipe=recipe)
    start = FLOAT_START["exp" if family == xs.EXPONENTIAL else recipe]
    params, _ = engine_params(model(family, start, prepare, **kw), family, x, start)
    ref, _, _ = restate(family, x, start, nats=False)
    ex = Exact(family, x, start)
    a_path = longest_path(n)
    worst = 0.0
    if family == xs.EXPONENTIAL:
        assert same_bits(params[0], ref[0])
        for i in positions(n):
            lam = ex.params(i)[1]
            err = abs(Fraction(float(params[1][i])) - lam)
            worst = max(worst, float(err / (a_path * EPS * lam)))
            assert err <= a_path * EPS * lam, (n, i, float(err), float(lam))
    else:
        assert same_bits(params[1], ref[1])
        for i in positions(n):
            mu, nu, lam = ex.params(i)
            beta = ex.beta(i)
            kn = Fraction(float(start[1])) + i
            beta_dev = kn / (kn + 1) * (nu / 2) / Fraction(float(params[2][i]))
            b_mu, b_beta = normal_bounds(x, start, i, a_path, mu, beta)
            e_mu, e_beta = abs(Fraction(float(params[0][i])) - mu), abs(beta_dev - beta)
            worst = max(worst, float(e_mu) / b_mu if b_mu else 0.0, float(e_beta) / b_beta)
            assert e_mu <= b_mu and e_beta <= b_beta, (recipe, n, i, float(e_mu), b_mu, float(e_beta), b_beta)
    print(f"float state family={family} n={n} {np.dtype(dtype).name} {recipe}: worst error / bound = {worst:.3g}")
    return worst


def check_against_loop(family, dtype, recipe, prepare, n=2000, **kw):
    """Issue test 3, last item: n = 2000 against the loop (c) with A replaced by n + A (the loop rounds once per value).
    Every recipe starts from hn_m = 0 here: the loop carries hn_m at the size of the data and rounds it once per value,
    an error of eps |x| that the bound covers through R = |hn_m - x_0| + ... only when the prior mean is that far from
    the data.  (With hn_m = 1e6 on the tight recipe the loop itself keeps eight digits of hn_beta, the pass all of them:
    there the pass is held to the exact oracle alone, check_float_state.)"""
    x = sample(family, n, seed=5, dtype=dtype, recipe=recipe)
    start = FLOAT_START["exp"] if family == xs.EXPONENTIAL else (0.0, 1.0, 1.0, 1.0)
    params, _ = engine_params(model(family, start, prepare, **kw), family, x, start)
    lm = model(family, start)
    hn = []
    for v in x:
        hn.append(hn_of(lm, family))
        lm.pred_and_update(float(v))
    a_path = n + longest_path(n)
    for i in range(n):
        if family == xs.EXPONENTIAL:
            assert abs(params[1][i] - hn[i][1]) <= a_path * EPS * hn[i][1]
        else:
            b_mu, b_beta = normal_bounds(x, start, i, a_path, hn[i][0], hn[i][3])
            kn = Fraction(float(start[1])) + i          # hn_beta behind the pass's p_lambda, in exact arithmetic
            beta_dev = kn / (kn + 1) * (Fraction(float(start[2])) + Fraction(i, 2)) / Fraction(float(params[2][i]))
            assert abs(params[0][i] - hn[i][0]) <= b_mu and abs(beta_dev - Fraction(float(hn[i][3]))) <= b_beta, (recipe, i)


def check_nats(family, x, start, prepare, **kw):
    """Issue test 4.  bernoulli: against the exact code length, 4 eps (1 + |nats|).  The others: against the mpmath formula
    at the pass's own returned parameters, 64 eps B.  ``loss=None`` gives the same bits.  Returns the worst error / bound."""
    params, code = engine_params(model(family, start, prepare, **kw), family, x, start)
    m = model(family, start, prepare, **kw)
    before = [getattr(m, k) for k in xs.PARAMS[family]]
    alone = m.pred_and_update_sequence(x, None, code_length=True)
    assert [getattr(m, k) for k in xs.PARAMS[family]] == before
    _, full = model(family, start, prepare, **kw).pred_and_update_sequence(x, code_length=True)
    assert same_bits(alone, code) and same_bits(full, code)
    ex = Exact(family, x, start) if family == xs.BERNOULLI else None
    worst = 0.0
    for i in positions(x.shape[0]):
        if family == xs.BERNOULLI:
            want, _ = nats_mp(family, ex.params(i), x[i])
            bound = 4 * EPS * (1 + abs(want))
        else:
            want, big = nats_mp(family, [p[i] for p in params], x[i], beta_i=np.float64(start[1]) + np.float64(i))
            bound = 64 * EPS * big
        err = abs(mp.mpf(float(code[i])) - want)
        worst = max(worst, float(err / bound))
        assert err <= bound, (family, i, float(err), float(bound))
    return worst


LONG_START = {xs.POISSON: (3.7e7, 1e7), xs.EXPONENTIAL: (1e7, 2.3e7), xs.NORMAL: (0.1, 1e7, 5e6, 4.9e6)}


# ---- categorical ------------------------------------------------------------------------------------------------------------
def cat_model(degree, alpha=None, prepare=None, **kw):
    from bayesml_amd import categorical
    m = categorical.LearnModel(degree, **kw)
    if alpha is not None:
        m.set_hn_params(np.asarray(alpha, dtype=np.float64))
    return prepare(m) if prepare is not None else m


def cat_sample(degree, n, seed=0, kind="random", dtype=np.int64):
    """Index samples: seeded draws, one category throughout, or a category that changes exactly at thread, wave and tile
    boundaries of the walk (256 positions a step, waves of 64)."""
    rng = np.random.default_rng(seed)
    if kind == "single":
        return np.full(n, degree - 1, dtype=dtype)
    if kind == "edges":
        cuts = sorted({c for c in (1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T, 2 * T + 64, 3 * T - 1, 3 * T) if c < n})
        x = np.zeros(n, dtype=dtype)
        for j, c in enumerate(cuts):
            x[c:] = (j + 1) % degree
        return x
    return rng.integers(0, degree, n).astype(dtype)


def cat_loop(degree, alpha, x, loss, onehot):
    """(predictions, nats, the model) of the per-value loop; x are indices."""
    m = cat_model(degree, alpha)
    eye = np.eye(degree, dtype=np.int64)
    preds, code = [], []
    for v in x:
        m.calc_pred_dist()
        code.append(-np.log(m._calc_pred_density(int(v))))
        preds.append(np.copy(m.pred_and_update(eye[int(v)] if onehot else int(v), loss, onehot)))
    return np.array(preds), np.array(code), m


def check_categorical_integer_state(degree, n, prepare, kind="random", with_loop=True, **kw):
    """Issue test 2 for the categorical family, index and one-hot form.  Dyadic prior arange(1, k + 1) / 2: every loss's
    predictions, the last p_theta_vec and hn_alpha_vec are the loop's bits.  Non-dyadic prior 0.3 + 0.7 sqrt(k): the rows
    are the restatement's bits and within 3 eps of the exact value."""
    x = cat_sample(degree, n, seed=n, kind=kind)
    eye = np.eye(degree, dtype=np.int64)
    alpha = np.arange(1, degree + 1) / 2.0
    if not with_loop:          # the last prediction's parameters: the last row, whatever the loss asked the pass for
        last_row = restate_categorical(x, False, alpha, "rows", False)[0][-1]
    for onehot in (False, True):
        xin = eye[x] if onehot else x
        for loss in ("squared", "0-1", "KL"):
            m = cat_model(degree, alpha, prepare, **kw)
            got = m.pred_and_update_sequence(xin, loss, onehot)
            if with_loop:
                preds, _, lm = cat_loop(degree, alpha, x, loss, onehot)
                assert got.dtype == preds.dtype and same_bits(got, preds), (degree, n, loss, onehot)
                assert same_bits(m.hn_alpha_vec, lm.hn_alpha_vec) and same_bits(m.p_theta_vec, lm.p_theta_vec)
            else:
                want, _, counts, _ = restate_categorical(x, False, alpha, "argmax" if loss == "0-1" else "rows", False)
                if loss == "0-1" and onehot:
                    want = eye[want]
                assert same_bits(got, want), (degree, n, loss, onehot)
                assert same_bits(m.hn_alpha_vec, alpha + counts)
                assert same_bits(m.p_theta_vec, last_row), (degree, n, loss, onehot)
    alpha = 0.3 + 0.7 * np.sqrt(np.arange(1, degree + 1))
    m = cat_model(degree, alpha, prepare, **kw)
    rows = m.pred_and_update_sequence(x, "squared", False)
    want, _, _, _ = restate_categorical(x, False, alpha, "rows", False)
    assert same_bits(rows, want) and same_bits(m.p_theta_vec, want[-1])
    s0 = Fraction(float(alpha.sum()))
    cum = np.cumsum(eye[x], axis=0) - eye[x]
    for i in positions(n, extra=16):
        for c in range(degree):
            e = (Fraction(float(alpha[c])) + int(cum[i, c])) / (s0 + i)
            assert abs(Fraction(float(rows[i, c])) - e) <= 3 * EPS * e, (degree, n, i, c)


def check_categorical_nats(degree, n, prepare, alpha=None, **kw):
    """Issue test 4: |nats - exact| <= 4 eps (1 + |nats|), the exact value from the binary64 S0 the pass is given; nats
    alone and nats of the full call are the same bits."""
    x = cat_sample(degree, n, seed=7)
    alpha = 0.3 + 0.7 * np.sqrt(np.arange(1, degree + 1)) if alpha is None else alpha
    m = cat_model(degree, alpha, prepare, **kw)
    before = m.p_theta_vec.copy()
    code = m.pred_and_update_sequence(x, None, False, code_length=True)
    assert same_bits(m.p_theta_vec, before)
    _, full = cat_model(degree, alpha, prepare, **kw).pred_and_update_sequence(x, "squared", False, code_length=True)
    _, hot = cat_model(degree, alpha, prepare, **kw).pred_and_update_sequence(np.eye(degree, dtype=np.int64)[x], "0-1", True,
                                                                              code_length=True)
    assert same_bits(code, full) and same_bits(code, hot)
    eye = np.eye(degree, dtype=np.int64)
    cum = np.cumsum(eye[x], axis=0) - eye[x]
    s0 = Fraction(float(alpha.sum()))
    worst = 0.0
    for i in positions(n):
        p = (Fraction(float(alpha[x[i]])) + int(cum[i, x[i]])) / (s0 + i)
        want = -mp.log(_mpf(p))
        bound = 4 * EPS * (1 + abs(want))
        err = abs(mp.mpf(float(code[i])) - want)
        worst = max(worst, float(err / bound))
        assert err <= bound, (degree, i)
    return worst


def check_categorical_rows_and_chunks(degree, n, prepare, kind="random", **kw):
    """Issue test 5: rows sum to one within 4 c_degree eps; the argmax is np.argmax of the rows; chunk lengths 1, 7, T and
    T + 1 give the unchunked call's bits in every output and in hn_alpha_vec, in ceil(n / m) passes."""
    x = cat_sample(degree, n, seed=degree, kind=kind, dtype=np.int32)
    alpha = 0.3 + 0.7 * np.sqrt(np.arange(1, degree + 1))
    ref = {}
    for loss in ("squared", "0-1"):
        m = cat_model(degree, alpha, prepare, **kw)
        ref[loss] = m.pred_and_update_sequence(x, loss, False, code_length=True) + (m.hn_alpha_vec.copy(), m.p_theta_vec.copy())
    rows, am = ref["squared"][0], ref["0-1"][0]
    assert rows.shape == (n, degree) and np.all(np.abs(rows.sum(axis=1) - 1.0) <= 4 * degree * EPS)
    assert am.dtype == np.int64 and np.array_equal(am, np.argmax(rows, axis=1))
    for length in (1, 7, T, T + 1):
        for loss in ("squared", "0-1"):
            m = cat_model(degree, alpha, prepare, **kw)
            got = m.pred_and_update_sequence(x, loss, False, code_length=True, chunk_bytes=8 * xs.work_len(xs.CATEGORICAL, degree, length))
            assert m._seq_pass().passes == -(-n // min(length, n)), (degree, length)
            for a, b in zip(got + (m.hn_alpha_vec, m.p_theta_vec), ref[loss]):
                assert same_bits(a, b), (degree, length, loss)


# ---- the reference's fixtures (tests/golden/make_golden_expfam_seq.py) ---------------------------------------------------------
FIXTURES = {"bernoulli": xs.BERNOULLI, "poisson": xs.POISSON, "exponential": xs.EXPONENTIAL, "normal": xs.NORMAL}


def check_fixture(name, fx, prepare, **kw):
    """Every recorded quantity of one scalar family's fixture.

    bernoulli, poisson (integer state, dyadic defaults): predictions of every loss and hn_* bit for bit; nats within the
    family's bound of test 4 plus the reference's own recorded error.
    exponential, normal: the loop rounds once per value, so parameters and the predictions that are parameters are held
    under the bounds of test 3 with A replaced by n + A; predictions computed from parameters under the same relative
    bound plus 4 eps for their own operations.  nats: the pass's nats are within 64 eps B of the formula at the pass's
    parameters (test 4) and the reference's within nats_err of the formula at its own; the two parameter sets differ by
    at most the bound just stated, and every term of the formula moves by at most max(|term|, 1) per unit of relative
    change of kappa, lambda, nu (and by 2 lambda |x - mu| per unit of mu), so the bound adds (n + A) eps (B + 1) and, for
    the normal family, 2 lambda |x - mu| times the bound on mu."""
    family = FIXTURES[name]
    for start in ("prior", "post"):
        x, hn0, hn1 = fx[start + "_x"], fx[start + "_hn0"], fx[start + "_hn1"]
        n = x.shape[0]
        a_path = n + longest_path(n)
        params, code = engine_params(model(family, hn0, prepare, **kw), family, x, hn0)
        for loss in LOSSES[family]:
            want = fx[f"{start}_pred_{loss.replace('-', '')}"]
            m = model(family, hn0, prepare, **kw)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got, nats = m.pred_and_update_sequence(x, loss, code_length=True)
            assert same_bits(nats, code)
            if family in (xs.BERNOULLI, xs.POISSON):
                assert same_bits(got, want), (name, start, loss)
                assert same_bits(hn_of(m, family), hn1)
            else:
                for i in range(n):
                    if family == xs.EXPONENTIAL:
                        # "abs" is lambda (2 ** (1 / kappa) - 1): an ulp of either side's pow is 1 / (2 ** (1 / kappa) - 1) ulps of it
                        rel = (a_path + 4) * EPS + (2 * EPS / (2.0 ** (1.0 / params[0][i]) - 1.0) if loss == "abs" else 0.0)
                        ok = (np.isnan(want[i]) and np.isnan(got[i])) or abs(got[i] - want[i]) <= rel * abs(want[i])
                    else:
                        ok = abs(got[i] - want[i]) <= normal_bounds(x, hn0, i, a_path, want[i], 0.0)[0]
                    assert ok, (name, start, loss, i, got[i], want[i])
                assert np.allclose(hn_of(m, family), hn1, rtol=(a_path + 16) * EPS, atol=0.0)
        for i in range(n):
            beta_i = np.float64(hn0[1]) + np.float64(i)
            exact, big = nats_mp(family, [p[i] for p in params], x[i], beta_i=beta_i)
            if family == xs.BERNOULLI:
                bound = 4 * EPS * (1 + abs(exact))
            elif family == xs.POISSON:
                bound = 64 * EPS * big
            else:
                bound = 64 * EPS * big + a_path * EPS * (big + 1)
                if family == xs.NORMAL:
                    mu, lam = float(params[0][i]), float(params[2][i])
                    bound += 2 * lam * abs(float(x[i]) - mu) * normal_bounds(x, hn0, i, a_path, mu, 0.0)[0]
            bound = float(bound) + float(fx[start + "_nats_err"][i])
            assert abs(code[i] - fx[start + "_nats"][i]) <= bound, (name, start, i, code[i], fx[start + "_nats"][i], bound)


def check_categorical_fixture(degree, fx, prepare, **kw):
    """The categorical fixtures (degrees 3 and 300, index and one-hot form).  The default prior 1/2 is dyadic: rows, argmax,
    one-hot predictions and hn_alpha_vec bit for bit; nats within 4 eps (1 + |nats|) plus one rounding of the reference's
    own log."""
    eye = np.eye(degree, dtype=np.int64)
    for start in ("prior", "post"):
        x, hn0, hn1 = fx[start + "_x"], fx[start + "_hn0"], fx[start + "_hn1"]
        for onehot in (False, True):
            for loss in ("squared", "0-1"):
                want = fx[f"{start}_pred_squared" if loss == "squared" else f"{start}_pred_01{'_onehot' if onehot else ''}"]
                m = cat_model(degree, hn0, prepare, **kw)
                got, nats = m.pred_and_update_sequence(eye[x] if onehot else x, loss, onehot, code_length=True)
                assert got.shape == want.shape and same_bits(got, want), (degree, start, onehot, loss)
                assert same_bits(m.hn_alpha_vec, hn1)
                ref = fx[start + "_nats"]
                assert np.all(np.abs(nats - ref) <= 4 * EPS * (1 + np.abs(ref)) + EPS * np.abs(ref))
