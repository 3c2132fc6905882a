"""Oracles for sequential prediction in linearregression / autoregressive (TEST INFRASTRUCTURE ONLY).

* ``block_form``: a NumPy restatement of the block form of DESIGN.md 4f "Sequential prediction" with the kernels' schedule
  (``schedule``, restated here, not imported) and their order of operations: per-block statistics, an exclusive scan in
  block order from a carry, the block-start state from the prefix, the block's marginal factor - in double-double
  (``dd_block_factor``) for the blocks the kernels take there: the first 2 D rows, and K_ii above ``DD_THRESHOLD``.
* ``row_loop``: the row-by-row loop from ``regression_oracle.update`` / ``pred_params`` (the reference's formulas in float64).
* ``ld_row_loop``: the same loop in ``numpy.longdouble`` with a plain Cholesky (restated from
  tests/golden/make_golden_regression.py): the "exact" value the tests compare against.
* ``CpuRegressionSeqPass``: CPU stand-in for ``bayesml_amd._regseq.RegressionSeqPass`` behind the private
  ``LearnModel._regseq_pass_factory`` seam; the product path never constructs it.
* ``errors`` / ``tolerance``: the measure and the bound every comparison uses.
* ``sweep`` and the small model helpers of the GPU tests.
"""
import numpy as np
import torch

import regression_oracle as orc

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
BLOCK = 64


# ---- the schedule ------------------------------------------------------------------------------------------------------------
def schedule(n, block=BLOCK):
    """Block bounds [0, 1, 3, 7, ..., block - 1, 2 block - 1, ..., n]: lengths 1, 2, ..., block / 2, block, ..., a tail."""
    bounds, length = [0], 1
    while bounds[-1] < n:
        bounds.append(min(n, bounds[-1] + length))
        length = min(2 * length, block)
    return bounds


# ---- code length ---------------------------------------------------------------------------------------------------------------
def _stirling_tail(x):
    r = 1.0 / x
    r2 = r * r
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))))


def lgamma_half_step(alpha):
    """lnGamma(a) - lnGamma(a + 1/2), as the kernel evaluates it: lgamma below 64, the Stirling difference from there."""
    from scipy.special import gammaln
    alpha = np.asarray(alpha, dtype=np.float64)
    small = gammaln(alpha) - gammaln(alpha + 0.5)
    a = np.maximum(alpha, 64.0)
    large = -(a * np.log1p(0.5 / a) + 0.5 * np.log(a) - 0.5 + (_stirling_tail(a + 0.5) - _stirling_tail(a)))
    return np.where(alpha < 64.0, small, large)


def nats_of(alpha, beta, p_lambda, v2):
    """-ln St(y | p_m, p_lambda, 2 alpha), v2 the squared whitened innovation: p_lambda (y - p_m)^2 / (2 alpha) = v2 / (2 beta)."""
    return (lgamma_half_step(alpha) + 0.5 * np.log(2.0 * np.pi * alpha / p_lambda)
            + (alpha + 0.5) * np.log1p(v2 / (2.0 * beta)))


def ld_lgamma_half_step(alpha):
    """The same difference in long double: shifted up to an argument >= 40 by the recurrence, then the Stirling series
    to x^-13 (next term below 1e-25)."""
    out = np.zeros(len(alpha), dtype=LD)
    for i, a in enumerate(np.asarray(alpha, dtype=LD)):
        shift = LD(0)
        while a < 40:
            shift += np.log((a + LD(0.5)) / a)          # lnG(a) - lnG(a + 1/2) = lnG(a + 1) - lnG(a + 3/2) + ln((a + 1/2) / a)
            a = a + 1

        def tail(x):
            r2 = 1 / (x * x)
            return (LD(1) / 12 + r2 * (-LD(1) / 360 + r2 * (LD(1) / 1260 + r2 * (-LD(1) / 1680 + r2 * (
                LD(1) / 1188 + r2 * (-LD(691) / 360360 + r2 * (LD(1) / 156))))))) / x
        out[i] = shift - (a * np.log1p(LD(0.5) / a) + LD(0.5) * np.log(a) - LD(0.5) + (tail(a + LD(0.5)) - tail(a)))
    return out


# ---- the block form ----------------------------------------------------------------------------------------------------------
def start_state(mu, lam, alpha, beta):
    lam, mu = np.asarray(lam, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    lm = lam @ mu
    return np.concatenate([lam.reshape(-1), lm, [mu @ lm, float(alpha), float(beta)]])


DD_THRESHOLD = 64.0        # csrc/regseq_kernels.h: kDdThreshold ("Double-double")


# ---- double-double, as csrc/regseq_kernels.h has it (a number is the pair hi, lo of float64 arrays) ---------------------
# (long double is not enough for K: its entries reach 1e6 and more where the Schur complements are of order one, and 64
# mantissa bits leave those 1e-13 off - the row loop in float64 has 1e-15)
def _dd_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _dd_add(a, b):
    hi, lo = _dd_sum(a[0], b[0])
    lo = lo + (a[1] + b[1])
    h = hi + lo
    return h, lo - (h - hi)


def _two_prod(a, b):
    """a b exactly (Veltkamp's split and Dekker's product, where the kernel has an fma)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    e = e + (a[0] * b[1] + a[1] * b[0])
    h = p + e
    return h, e - (h - p)


def _dd_neg(a):
    return -a[0], -a[1]


def _dd_div(a, b):
    zero = np.zeros_like(b[0])
    q1 = a[0] / b[0]
    r = _dd_add(a, _dd_neg(_dd_mul((q1, zero), b)))
    q2 = r[0] / b[0]
    r = _dd_add(r, _dd_neg(_dd_mul((q2, zero), b)))
    q3 = r[0] / b[0]
    return _dd_add(_dd_sum(q1, q2), (q3, zero))


def _dd_sqrt(a):
    x = np.sqrt(a[0])
    zero = np.zeros_like(x)
    r = _dd_add(a, _dd_neg(_dd_mul((x, zero), (x, zero))))
    return _dd_sum(x, r[0] / (2.0 * x))


def dd_block_factor(z):
    """The factor R of K = I + z z^T as the kernel's double-double path forms it: K summed column of z by column of z from
    error-free products, then the right-looking Cholesky of ``dd_cholesky_packed``; the high words of R."""
    z = np.asarray(z, dtype=np.float64)
    m = z.shape[0]
    k = (np.eye(m), np.zeros((m, m)))
    for c in range(z.shape[1]):
        k = _dd_add(k, _two_prod(z[:, c, None], z[None, :, c]))
    hi, lo = k
    for j in range(m):
        d = _dd_sqrt((hi[j, j], lo[j, j]))
        col = _dd_div((hi[j + 1:, j], lo[j + 1:, j]), (np.full(m - j - 1, d[0]), np.full(m - j - 1, d[1])))
        hi[j, j], lo[j, j] = d
        hi[j + 1:, j], lo[j + 1:, j] = col
        upd = _dd_mul((-col[0][:, None], -col[1][:, None]), (col[0][None, :], col[1][None, :]))
        hi[j + 1:, j + 1:], lo[j + 1:, j + 1:] = _dd_add((hi[j + 1:, j + 1:], lo[j + 1:, j + 1:]), upd)
    return np.tril(hi)


def block_form(w, y, start, blocks_per_pass=None, dd_threshold=DD_THRESHOLD, diag=None):
    """(p_ms, p_lambdas, p_nus, nats) of the rows w [n, D], targets y [n], from the state ``start`` (``start_state``).
    ``blocks_per_pass``: cut the call into passes of so many blocks, carrying [G | c | s | n] between them.
    ``dd_threshold``: None takes the data out of the double-double decision (the form before the criterion existed).
    ``diag``: a list that receives (first row, end, starts within the first 2 D rows, max_i K_ii) of every block."""
    from scipy.linalg import solve_triangular
    w, y = np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, D = w.shape
    lam0, lm0 = start[:D * D].reshape(D, D), start[D * D:D * D + D]
    m0, alpha0, beta0 = start[D * D + D:]
    bounds = schedule(n)
    nb = len(bounds) - 1
    per = nb if blocks_per_pass is None else blocks_per_pass
    out = [np.zeros(n) for _ in range(4)]
    carry = [np.zeros((D, D)), np.zeros(D), 0.0, 0.0]
    for b0 in range(0, nb, per):
        ids = range(b0, min(b0 + per, nb))
        stats = []
        for b in ids:                                                    # (1) per-block statistics
            wb, yb = w[bounds[b]:bounds[b + 1]], y[bounds[b]:bounds[b + 1]]
            stats.append((wb.T @ wb, wb.T @ yb, yb @ yb, float(len(yb))))
        prefix = []
        for st in stats:                                                 # (2) exclusive scan, in block order
            prefix.append(tuple(carry))
            carry = [c + s for c, s in zip(carry, st)]
        for b, (g, c, s, rows_before) in zip(ids, prefix):
            low = np.linalg.cholesky(lam0 + g)                           # (3) the state at the block's first row
            linv = np.tril(solve_triangular(low, np.eye(D), lower=True))
            u = solve_triangular(low, lm0 + c, lower=True)               # (by substitution: the explicit inverse serves Z alone)
            mu_c = solve_triangular(low.T, u, lower=False)
            beta_c = beta0 + ((s + m0) - u @ u) / 2.0
            lo, hi = bounds[b], bounds[b + 1]                            # (4) the block's innovations
            z = w[lo:hi] @ linv.T
            k = np.eye(hi - lo) + z @ z.T
            k_max = float(np.max(np.diag(k)))
            if diag is not None:
                diag.append((lo, hi, rows_before < 2 * D, k_max))
            # K and its factor in double-double for a block of the first 2 D rows, and for one whose binary64 K has a
            # diagonal entry above the threshold: a function of the block's rows and start state
            if rows_before < 2 * D or (dd_threshold is not None and k_max > dd_threshold):
                r = dd_block_factor(z)
            else:
                r = np.linalg.cholesky(k)
            v = solve_triangular(r, y[lo:hi] - w[lo:hi] @ mu_c, lower=True)
            v2 = v * v
            before = np.concatenate([[0.0], np.cumsum(v2)[:-1]])
            alpha = alpha0 + (rows_before + np.arange(hi - lo)) / 2.0
            beta = beta_c + before / 2.0
            rii = np.diag(r)
            out[0][lo:hi] = y[lo:hi] - rii * v
            out[1][lo:hi] = alpha / (beta * (rii * rii))
            out[2][lo:hi] = 2.0 * alpha
            out[3][lo:hi] = nats_of(alpha, beta, out[1][lo:hi], v2)
    return tuple(out)


# ---- the loops ---------------------------------------------------------------------------------------------------------------
def row_loop(w, y, mu, lam, alpha, beta):
    """The reference's loop in float64: (p_ms, p_lambdas, p_nus, nats, final state)."""
    from scipy.stats import t as student
    w, y = np.asarray(w, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(y)
    out = [np.zeros(n) for _ in range(4)]
    for i in range(n):
        pm, pl, pn = orc.pred_params(mu, lam, alpha, beta, w[i:i + 1])
        out[0][i], out[1][i], out[2][i] = pm[0], pl[0], pn[0]
        mu, lam, alpha, beta = orc.update(mu, lam, alpha, beta, w[i:i + 1], y[i:i + 1])
    out[3][:] = -student.logpdf(y, loc=out[0], scale=1.0 / np.sqrt(out[1]), df=out[2])
    return (*out, (mu, lam, alpha, beta))


def ld_cholesky(a):
    a = np.array(a, dtype=LD)
    n = a.shape[0]
    low = np.zeros((n, n), dtype=LD)
    for j in range(n):
        low[j, j] = np.sqrt(a[j, j] - low[j, :j] @ low[j, :j])
        if j + 1 < n:
            low[j + 1:, j] = (a[j + 1:, j] - low[j + 1:, :j] @ low[j, :j]) / low[j, j]
    return low


def ld_forward(low, b):
    """low^-1 b for lower triangular low."""
    z = np.zeros(len(b), dtype=LD)
    for j in range(len(b)):
        z[j] = (b[j] - low[j, :j] @ z[:j]) / low[j, j]
    return z


def ld_row_loop(w, y, mu, lam, alpha, beta, rows=None):
    """The loop in long double, as statistics (the state before row i is a function of the sums over the rows before it, so
    nothing accumulates but those sums): (p_ms, p_lambdas, p_nus, nats).  ``rows``: the rows to predict (all of them if
    None); the sums run over every row, the factorisation only at those, and the other rows' outputs are NaN."""
    w, y = np.asarray(w, dtype=np.float64).astype(LD), np.asarray(y, dtype=np.float64).astype(LD)
    n, D = w.shape
    lam0, mu0 = np.array(lam, dtype=LD), np.array(mu, dtype=LD)
    alpha0, beta0 = LD(alpha), LD(beta)
    lm0, m0 = lam0 @ mu0, mu0 @ lam0 @ mu0
    g, c, s = np.zeros((D, D), dtype=LD), np.zeros(D, dtype=LD), LD(0)
    out = [np.zeros(n, dtype=LD) for _ in range(4)]
    wanted = np.ones(n, dtype=bool)
    if rows is not None:
        wanted[:] = False
        wanted[np.asarray(rows, dtype=np.int64)] = True
        for o in out:
            o[~wanted] = np.nan
    for i in range(n):
        if wanted[i]:
            low = ld_cholesky(lam0 + g)
            u = ld_forward(low, lm0 + c)
            q = ld_forward(low, w[i])
            a_i = alpha0 + LD(i) / 2
            b_i = beta0 + (s + m0 - u @ u) / 2
            out[0][i] = q @ u                               # w . mu = (L^-1 w) . (L^-1 r)
            out[1][i] = a_i / b_i / (1 + q @ q)
            out[2][i] = 2 * a_i
        g += np.outer(w[i], w[i])
        c += w[i] * y[i]
        s += y[i] * y[i]
    e2 = out[1][wanted] * (y[wanted] - out[0][wanted]) ** 2 / out[2][wanted]
    half = out[2][wanted] / 2
    out[3][wanted] = (ld_lgamma_half_step(half) + np.log(2 * LD(np.pi) * half / out[1][wanted]) / 2
                      + (half + LD(0.5)) * np.log1p(e2))
    return tuple(out)


# ---- the measure and the bound -------------------------------------------------------------------------------------------
NAMES = ("p_m", "p_lambda", "p_nu", "nats")


def errors(got, exact, y, rows=slice(None)):
    """Worst error per output over ``rows``: p_m relative to max |y|, p_lambda and p_nu relative per row, nats relative
    per row with the magnitude floored at 1 (a code length is a sum of logarithms of order one and may pass through 0)."""
    ymax = LD(np.max(np.abs(y)))
    res = {}
    for name, a, b in zip(NAMES, got, exact):
        a, b = np.asarray(a).astype(LD)[rows], np.asarray(b, dtype=LD)[rows]
        if a.size == 0:
            res[name] = 0.0
            continue
        den = ymax if name == "p_m" else (np.maximum(np.abs(b), 1) if name == "nats" else np.abs(b))
        res[name] = float(np.max(np.abs(a - b) / den))
    return res


def tolerance(ref_err):
    """8 x the reference loop's own error on the same rows (the block form sums B + D terms where the loop's solve sums
    D), never below 64 eps."""
    return {k: max(8.0 * v, 64.0 * EPS) for k, v in ref_err.items()}


def check(label, got, exact, ref, y, D, rows=None):
    """Holds ``got`` to the bound, separately on the first 2 D rows and on the rest; prints worst error / tolerance.
    ``ref``: the reference loop's outputs on the same rows, or a dict {"head": errors, "rest": errors} recorded earlier.
    ``rows``: the row numbers to compare (``ld_row_loop``'s ``rows``), all of them if None."""
    worst = 0.0
    parts = (slice(0, 2 * D), slice(2 * D, None))
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        parts = (rows[rows < 2 * D], rows[rows >= 2 * D])
    for part, rows in zip(("head", "rest"), parts):
        ref_err = ref[part] if isinstance(ref, dict) else errors(ref, exact, y, rows)
        tol, err = tolerance(ref_err), errors(got, exact, y, rows)
        ratios = {k: err[k] / tol[k] for k in err}
        print(f"{label} [{part}]: " + ", ".join(f"{k} {err[k]:.1e} / {tol[k]:.1e}" for k in err))
        worst = max(worst, max(ratios.values()))
        assert max(ratios.values()) <= 1.0, (label, part, err, tol)
    return worst


FIXTURES = [f"regression_seq_{m}_{kind}.npz" for m in ("linreg_d1", "linreg_d3", "linreg_d17", "ar_p0", "ar_p1", "ar_p4")
            for kind in ("default", "diffuse", "posterior")]


def fixture_parts(g):
    """(w, y, start state as (mu, lam, alpha, beta), long-double traces, the reference's recorded errors) of a fixture
    of tests/golden/make_golden_regression_seq.py."""
    w, y = orc.lag_matrix(g["x"], int(g["p"]), None) if "p" in g else (g["x"], g["y"])
    start = (g["start_mu_vec"], g["start_lambda_mat"], float(g["start_alpha"]), float(g["start_beta"]))
    exact = [g["exact_" + k] for k in NAMES]
    ref = {part: dict(zip(NAMES, g["ref_vs_exact_" + part])) for part in ("head", "rest")}
    return w, y, start, exact, ref


# ---- the seam ----------------------------------------------------------------------------------------------------------------
class CpuRegressionSeqPass:
    def __init__(self, D, blocks_per_pass=None):
        self.D = D
        self.device = torch.device("cpu")
        self.blocks_per_pass = blocks_per_pass
        self.launch_info = "cpu stand-in"

    def adopt(self, a):
        from bayesml_amd._regression import adopt_tensor
        return adopt_tensor(a, self.device)

    def _out(self, w, y, start, want_nats):
        pm, pl, _pn, nats = block_form(w, y, np.asarray(start, dtype=np.float64), self.blocks_per_pass)
        return torch.from_numpy(pm), torch.from_numpy(pl), torch.from_numpy(nats) if want_nats else None

    def run(self, x, y, start, want_nats, chunk_bytes=None):
        from bayesml_amd._regression import _code
        assert x.dim() == 2 and x.shape[1] == self.D and y.shape == (x.shape[0],)
        self.last_dtypes = (_code(x.dtype), _code(y.dtype))
        return self._out(x.to(torch.float64).numpy(), y.to(torch.float64).numpy(), start, want_nats)

    def run_window(self, series, padding, start, want_nats, chunk_bytes=None):
        assert series.dim() == 1 and padding in (0, 1)
        w, y = orc.lag_matrix(series.to(torch.float64).numpy(), self.D - 1, "zeros" if padding == 1 else None)
        return self._out(w, y, start, want_nats)

    def close(self):
        pass


def cpu_seq_factory(D):
    return CpuRegressionSeqPass(D)


def stand_ins(m):
    from fake_regression_engine import cpu_factory
    m._reg_pass_factory = cpu_factory
    m._regseq_pass_factory = cpu_seq_factory
    return m


def model_of(g, start, real=False):
    """The LearnModel of a fixture at its start state (on the stand-ins unless ``real``) and the call's arguments."""
    from bayesml_amd import autoregressive as ar, linearregression as lr
    if "p" in g:
        m, args = ar.LearnModel(int(g["p"])), (g["x"],)
    else:
        m, args = lr.LearnModel(int(g["D"])), (g["x"], g["y"])
    m.set_hn_params(*start)
    return (m if real else stand_ins(m)), args


# ---- the models on the device (the GPU tests' helpers) ----------------------------------------------------------------------
DEFAULT = lambda D: (np.zeros(D), np.eye(D), 1.0, 1.0)      # noqa: E731
HN = ("hn_mu_vec", "hn_lambda_mat", "hn_alpha", "hn_beta")


def dev():
    return torch.device("cuda", 0)


def linreg(D, start=None):
    from bayesml_amd import linearregression as lr
    m = lr.LearnModel(D, device=dev())
    return m if start is None else m.set_hn_params(*start)


def autoreg(p, start=None):
    from bayesml_amd import autoregressive as ar
    m = ar.LearnModel(p, device=dev())
    return m if start is None else m.set_hn_params(*start)


def hn_equal(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in HN)


def synth(D, n, seed, intercept=0.0):
    x, y, _ = orc.synth_linreg(D, n, seed, 2.0, np.float64)
    return x, y + intercept


def budget_for(D, blocks):
    """chunk_bytes that makes a pass hold so many blocks."""
    from bayesml_amd import _regseq
    return 8 * _regseq.work_slots(D, blocks)


def sweep(label, make, rows_of, ns, w, y, start, rows=None):
    """Every n of ``ns`` is a call on the first n rows; the loops run once, on the longest: prediction i does not depend on
    the rows after i.  ``rows``: the rows the long-double loop predicts and the comparison looks at (all if None)."""
    D = w.shape[1]
    exact = ld_row_loop(w, y, *start, rows=rows)
    ref = row_loop(w, y, *start)[:4]
    worst = 0.0
    for n in ns:
        m = make()
        pred, nats = m.pred_and_update_sequence(*rows_of(n), code_length=True)
        got = (pred, m.p_lambdas, m.p_nus, nats)
        assert all(a.shape == (n,) for a in got)
        sub = None if rows is None else [i for i in rows if i < n]
        worst = max(worst, check(f"{label} n = {n}", got, [e[:n] for e in exact], [r[:n] for r in ref], y[:n], D, rows=sub))
        assert hn_equal(m, make().update_posterior(*rows_of(n)))
    print(f"{label}: worst error / tolerance {worst:.2f}")
    return worst
