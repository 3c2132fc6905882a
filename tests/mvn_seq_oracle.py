"""Oracles for sequential prediction in multivariate_normal (TEST INFRASTRUCTURE ONLY).

* ``block_form``: a NumPy restatement of the block form of DESIGN.md 4f "Sequential prediction, multivariate normal" with
  the kernels' schedule (``schedule``, restated here) and their order of operations: per-block column sums about the pivot and their exclusive scan from a carry, the
  pivot-relative means, the innovation rows, the per-block Grams and their scan, the block-start factor, the block's
  marginal factor - in double-double for the blocks the kernels take there: the first 2 D rows, and K_ii above
  ``DD_THRESHOLD`` - and the closing formulas.
* ``row_loop``: the reference's formulas in float64 row by row, its ``inv`` per row and scipy's ``multivariate_t`` included.
* ``ld_row_loop``: the same loop in ``numpy.longdouble``: the means from the column sums, S by adding the innovation
  products (no cancelling term), a plain Cholesky at the rows asked for: the "exact" value the tests compare against.
* ``errors`` / ``tolerance`` / ``check``: the measure and the bound every comparison uses (regression_seq_oracle's rule).
* ``log_marginal``: ln p(X) of a sample between two states, for the sum of the code lengths.
* ``CpuMvnSeqPass``: CPU stand-in for ``bayesml_amd._mvnseq.MvnSeqPass`` behind the private
  ``LearnModel._mvnseq_pass_factory`` seam; the product path never constructs it.
* ``sweep`` / ``synth`` / ``model`` / ``budget_for``: what the GPU tests share (``sweep`` also runs on the stand-in).
"""
import numpy as np
import torch

import regression_seq_oracle as rseq

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
BLOCK = 64
DD_THRESHOLD = 64.0        # csrc/regseq_kernels.h: kDdThreshold
NAMES = ("p_m", "p_v_logdet", "p_quad", "nats")


# ---- the schedule ------------------------------------------------------------------------------------------------------------
def schedule(n, block=BLOCK):
    """Block bounds [0, 1, 3, 7, ..., block - 1, 2 block - 1, ..., n]: lengths 1, 2, ..., block / 2, block, ..., a tail."""
    bounds, length = [0], 1
    while bounds[-1] < n:
        bounds.append(min(n, bounds[-1] + length))
        length = min(2 * length, block)
    return bounds


def work_slots(D, blocks, block=BLOCK):
    """Doubles of a pass's workspace (csrc/mvnseq.hip: layout_of), restated."""
    tiles = 2 * ((D + 31) // 32)
    pd = 16 * ((D + 15) // 16)
    per_block = pd + block + block * D + (tiles * (tiles + 1) // 2 * 256 + 16 * tiles + 16) + (pd * pd + pd + 2)
    return blocks + 1 + blocks * per_block


# ---- code length ---------------------------------------------------------------------------------------------------------------
def lgamma_step(a, h):
    """lnGamma(a) - lnGamma(a + h) as the kernel evaluates it: lgamma below 64, the Stirling difference from there."""
    from scipy.special import gammaln
    a = np.asarray(a, dtype=np.float64)
    small = gammaln(a) - gammaln(a + h)
    b = np.maximum(a, 64.0)
    large = -((b - 0.5) * np.log1p(h / b) + h * np.log(b + h) - h + (rseq._stirling_tail(b + h) - rseq._stirling_tail(b)))
    return np.where(a < 64.0, small, large)


def ld_lgamma(x):
    """lnGamma in long double: shifted up to an argument >= 40 by the recurrence, then the Stirling series to x^-13."""
    x = np.array(x, dtype=LD)
    shift = np.zeros_like(x)
    for _ in range(40):
        low = x < 40
        shift = np.where(low, shift + np.log(np.where(low, x, 1)), shift)
        x = np.where(low, x + 1, x)
    r2 = 1 / (x * x)
    tail = (LD(1) / 12 + r2 * (-LD(1) / 360 + r2 * (LD(1) / 1260 + r2 * (-LD(1) / 1680 + r2 * (
        LD(1) / 1188 + r2 * (-LD(691) / 360360 + r2 * (LD(1) / 156))))))) / x
    return (x - LD(0.5)) * np.log(x) - x + np.log(2 * LD(np.pi)) / 2 + tail - shift


def closing(D, kappa, p_nu, logdet_s, q, lgstep, log=np.log, log1p=np.log1p, pi=np.pi):
    """(ln det p_v_mat, quad, nats) from kappa_i, p_nu, ln det S_i and q_i = u_i^T S_i^-1 u_i."""
    logdet_v = D * log(kappa * p_nu / (kappa + 1)) - logdet_s
    h = D / 2
    nats = lgstep + h * log(pi * p_nu) - logdet_v / 2 + (p_nu / 2 + h) * log1p(q)
    return logdet_v, p_nu * q, nats


# ---- the block form ----------------------------------------------------------------------------------------------------------
def start_state(s0, m0, kappa0, nu0):
    return np.concatenate([np.asarray(s0, dtype=np.float64).reshape(-1), np.asarray(m0, dtype=np.float64),
                           [float(kappa0), float(nu0)]])


def dd_block_factor(z):
    """The factor R of K = I + z z^T as the kernel's double-double path forms it (regression_seq_oracle.dd_block_factor),
    both words: (hi, lo)."""
    z = np.asarray(z, dtype=np.float64)
    m = z.shape[0]
    k = (np.eye(m), np.zeros((m, m)))
    for c in range(z.shape[1]):
        k = rseq._dd_add(k, rseq._two_prod(z[:, c, None], z[None, :, c]))
    hi, lo = k
    for j in range(m):
        d = rseq._dd_sqrt((hi[j, j], lo[j, j]))
        col = rseq._dd_div((hi[j + 1:, j], lo[j + 1:, j]), (np.full(m - j - 1, d[0]), np.full(m - j - 1, d[1])))
        hi[j, j], lo[j, j] = d
        hi[j + 1:, j], lo[j + 1:, j] = col
        upd = rseq._dd_mul((-col[0][:, None], -col[1][:, None]), (col[0][None, :], col[1][None, :]))
        hi[j + 1:, j + 1:], lo[j + 1:, j + 1:] = rseq._dd_add((hi[j + 1:, j + 1:], lo[j + 1:, j + 1:]), upd)
    return np.tril(hi), np.tril(lo)


def block_form(x, start, blocks_per_pass=None, dd_threshold=DD_THRESHOLD, diag=None, carry_out=None):
    """(p_m_vecs [n, D], p_nus, p_v_logdets, p_quads, nats) of the rows x [n, D] from the state ``start``
    (``start_state``).  ``blocks_per_pass``: cut the call into passes of so many blocks, carrying [G | sum | n] between
    them.  ``diag``: a list that receives (first row, end, starts within the first 2 D rows, max_i K_ii) of every block.
    ``carry_out``: a list that receives the carry [G | sum (x - pivot) | n] after the last pass."""
    from scipy.linalg import solve_triangular
    x = np.asarray(x, dtype=np.float64)
    n, D = x.shape
    s0, m0 = start[:D * D].reshape(D, D), start[D * D:D * D + D]
    kappa0, nu0 = start[D * D + D:]
    bounds = schedule(n)
    nb = len(bounds) - 1
    per = nb if blocks_per_pass is None else blocks_per_pass
    pivot = x[0].copy()
    d = x - pivot
    base = kappa0 * (m0 - pivot)
    means, logdets, quads, nats = np.zeros((n, D)), np.zeros(n), np.zeros(n), np.zeros(n)
    idx = np.arange(n, dtype=np.float64)
    kappa = kappa0 + idx
    p_nus = ((nu0 + idx) - D) + 1.0
    c_g, c_s, c_n = np.zeros((D, D)), np.zeros(D), 0.0
    for b0 in range(0, nb, per):
        ids = list(range(b0, min(b0 + per, nb)))
        before = []
        for b in ids:                                                    # (1), (2) column sums, scanned in block order
            before.append(c_s)
            blk = d[bounds[b]:bounds[b + 1]]
            c_s = c_s + (np.cumsum(blk, axis=0)[-1] if len(blk) else 0.0)
        us, grams = [], []
        for b, bef in zip(ids, before):                                  # (3), (4) means, innovation rows, Grams
            lo, hi = bounds[b], bounds[b + 1]
            inblk = np.concatenate([np.zeros((1, D)), np.cumsum(d[lo:hi], axis=0)[:-1]])
            m_rel = (base + (bef + inblk)) / kappa[lo:hi, None]
            means[lo:hi] = pivot + m_rel
            u = np.sqrt(kappa[lo:hi] / (kappa[lo:hi] + 1.0))[:, None] * (d[lo:hi] - m_rel)
            us.append(u)
            grams.append(u.T @ u)
        prefix = []
        for g in grams:                                                  # (5) exclusive scan, in block order
            prefix.append(c_g)
            c_g = c_g + g
        c_n += bounds[ids[-1] + 1] - bounds[ids[0]]
        for b, u, g in zip(ids, us, prefix):
            lo, hi = bounds[b], bounds[b + 1]
            low = np.linalg.cholesky(s0 + g)                             # (6) the state at the block's first row
            sumlog = np.sum(np.log(np.diag(low)))
            linv = np.tril(solve_triangular(low, np.eye(D), lower=True))
            z = u @ linv.T                                               # (7) the block's innovations
            zz = np.sum(z * z, axis=1)
            k_max = float(np.max(1.0 + zz))
            head = lo < 2 * D
            if diag is not None:
                diag.append((lo, hi, head, k_max))
            if head or (dd_threshold is not None and k_max > dd_threshold):
                rh, rl = dd_block_factor(z)
                r = (np.diag(rh).copy(), np.diag(rl).copy())
                q = rseq._dd_add(rseq._dd_mul(r, r), (np.full(hi - lo, -1.0), np.zeros(hi - lo)))[0]
            else:
                r = np.linalg.cholesky(np.eye(hi - lo) + z @ z.T)
                q = zz - np.array([np.sum(r[i, :i] ** 2) for i in range(hi - lo)])
            q = np.maximum(q, 0.0)
            lq = np.log1p(q)
            logdet_s = 2.0 * sumlog + np.concatenate([[0.0], np.cumsum(lq)[:-1]])
            logdets[lo:hi], quads[lo:hi], nats[lo:hi] = closing(
                D, kappa[lo:hi], p_nus[lo:hi], logdet_s, q, lgamma_step(0.5 * p_nus[lo:hi], 0.5 * D))
    if carry_out is not None:
        carry_out.append(np.concatenate([c_g.reshape(-1), c_s, [c_n]]))
    return means, p_nus, logdets, quads, nats


# ---- the loops ---------------------------------------------------------------------------------------------------------------
def row_loop(x, m, kappa, nu, w_inv, rows=None):
    """The reference's loop in float64 (bayesml/multivariate_normal/_multivariatenormal.py: calc_pred_dist :687-693,
    make_prediction's multivariate_t, update_posterior :501-524 with one row, its ``inv`` included):
    (p_m_vecs, p_nus, p_v_logdets, p_quads, nats, final state (m, kappa, nu, w_inv)).  ``rows``: the rows to predict (all
    if None); the state is updated at every row - that recursion does not read the inverse - and the predicted rows'
    outputs are the full loop's bits, the others' p_v_logdets, p_quads and nats NaN."""
    from scipy.stats import multivariate_t
    x = np.asarray(x, dtype=np.float64)
    n, D = x.shape
    m, w_inv = np.array(m, dtype=np.float64), np.array(w_inv, dtype=np.float64)
    kappa, nu = float(kappa), float(nu)
    wanted = np.ones(n, dtype=bool)
    if rows is not None:
        wanted[:] = False
        wanted[np.asarray(rows, dtype=np.int64)] = True
    means, p_nus = np.zeros((n, D)), np.zeros(n)
    logdets, quads, nats = (np.full(n, np.nan) for _ in range(3))
    for i in range(n):
        p_nu = nu - D + 1
        means[i], p_nus[i] = m, p_nu
        diff = x[i] - m
        if wanted[i]:
            w = np.linalg.inv(w_inv)
            p_v = kappa * p_nu / (kappa + 1) * w
            p_v_inv = (kappa + 1) / kappa / p_nu * w_inv
            logdets[i] = np.linalg.slogdet(p_v)[1]
            quads[i] = diff @ p_v @ diff
            nats[i] = -multivariate_t.logpdf(x[i], loc=m, shape=p_v_inv, df=p_nu)
        w_inv = w_inv + diff[:, None] @ diff[None, :] * kappa / (kappa + 1)          # (x_bar = x_i, the scatter is zero)
        m = (kappa * m + x[i]) / (kappa + 1)
        kappa += 1
        nu += 1
    return means, p_nus, logdets, quads, nats, (m, kappa, nu, w_inv)


def ld_row_loop(x, m, kappa, nu, w_inv, rows=None):
    """The loop in long double: the mean before row i from the column sums (about row 0, so that nothing cancels in them),
    S by adding the innovation products, a plain Cholesky at the rows asked for: (p_m_vecs, p_nus, p_v_logdets, p_quads,
    nats).  ``rows``: the rows to predict (all of them if None); the sums run over every row, the other rows' outputs
    are NaN."""
    x64 = np.asarray(x, dtype=np.float64)
    n, D = x64.shape
    x = x64.astype(LD)
    pivot = x[0].copy()
    m0, s = np.array(m, dtype=LD), np.array(w_inv, dtype=LD)
    kappa0, nu0 = LD(kappa), LD(nu)
    wanted = np.ones(n, dtype=bool)
    if rows is not None:
        wanted[:] = False
        wanted[np.asarray(rows, dtype=np.int64)] = True
    means = np.full((n, D), np.nan, dtype=LD)
    p_nus, logdet_s, q = (np.full(n, np.nan, dtype=LD) for _ in range(3))
    a = np.zeros(D, dtype=LD)
    for i in range(n):
        k = kappa0 + i
        m_rel = (kappa0 * (m0 - pivot) + a) / k
        u = np.sqrt(k / (k + 1)) * ((x[i] - pivot) - m_rel)
        if wanted[i]:
            low = rseq.ld_cholesky(s)
            v = rseq.ld_forward(low, u)
            means[i] = pivot + m_rel
            p_nus[i] = nu0 + i - D + 1
            logdet_s[i] = 2 * np.sum(np.log(np.diag(low)))
            q[i] = v @ v
        s = s + np.outer(u, u)
        a = a + (x[i] - pivot)
    kap = kappa0 + np.arange(n).astype(LD)
    half = D / LD(2)
    safe = np.where(wanted, p_nus, 1)
    lgstep = ld_lgamma(safe / 2) - ld_lgamma(safe / 2 + half)
    logdets, quads, nats = closing(LD(D), kap, p_nus, logdet_s, q, lgstep, pi=LD(np.pi))
    return means, p_nus, logdets, quads, nats


def ld_carry(x, m, kappa, nu, w_inv):
    """[G | sum (x - pivot) | n] after all rows, in long double: G the Gram matrix of the innovation rows."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n, D = x.shape
    pivot, m0, kappa0 = x[0].copy(), np.array(m, dtype=LD), LD(kappa)
    g, a = np.zeros((D, D), dtype=LD), np.zeros(D, dtype=LD)
    for i in range(n):
        k = kappa0 + i
        u = np.sqrt(k / (k + 1)) * ((x[i] - pivot) - (kappa0 * (m0 - pivot) + a) / k)
        g += np.outer(u, u)
        a += x[i] - pivot
    return np.concatenate([g.reshape(-1), a, [LD(n)]])


def log_marginal(D, n, kappa0, nu0, w_inv0, kappa_n, nu_n, w_inv_n):
    """ln p(X) of n rows between the states 0 and n:
    -(n D / 2) ln pi + (D / 2) ln(kappa_0 / kappa_n) + lnGamma_D(nu_n / 2) - lnGamma_D(nu_0 / 2)
    + (nu_0 / 2) ln det S_0 - (nu_n / 2) ln det S_n;  also the terms, for the magnitude summed."""
    from scipy.special import multigammaln
    terms = [-(n * D / 2.0) * np.log(np.pi), (D / 2.0) * np.log(kappa0 / kappa_n), multigammaln(nu_n / 2.0, D),
             -multigammaln(nu0 / 2.0, D), (nu0 / 2.0) * np.linalg.slogdet(w_inv0)[1],
             -(nu_n / 2.0) * np.linalg.slogdet(w_inv_n)[1]]
    return float(np.sum(terms)), terms


# ---- the measure and the bound -------------------------------------------------------------------------------------------
def errors(got, exact, x, rows=slice(None)):
    """Worst error per output over ``rows``; ``got`` and ``exact`` are (p_m_vecs, p_v_logdets, p_quads, nats): the means
    relative to max |x|, p_quads relative per row, p_v_logdets and nats relative per row with the magnitude floored at 1."""
    xmax = LD(np.max(np.abs(x)))
    res = {}
    for name, a, b in zip(NAMES, got, exact):
        a, b = np.asarray(a).astype(LD)[rows], np.asarray(b, dtype=LD)[rows]
        if a.size == 0:
            res[name] = 0.0
            continue
        den = xmax if name == "p_m" else (np.abs(b) if name == "p_quad" else np.maximum(np.abs(b), 1))
        res[name] = float(np.max(np.abs(a - b) / den))
    return res


def tolerance(ref_err):
    """8 x the reference loop's own error on the same rows, never below 64 eps (regression_seq_oracle.tolerance)."""
    return {k: max(8.0 * v, 64.0 * EPS) for k, v in ref_err.items()}


def check(label, got, exact, ref, x, D, rows=None):
    """Holds ``got`` to the bound, separately on the first 2 D rows and on the rest; prints worst error / tolerance.
    ``ref``: the reference loop's outputs on the same rows, or a dict {"head": errors, "rest": errors} recorded earlier.
    ``rows``: the row numbers to compare (``ld_row_loop``'s ``rows``), all of them if None."""
    worst = 0.0
    parts = (slice(0, 2 * D), slice(2 * D, None))
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        parts = (rows[rows < 2 * D], rows[rows >= 2 * D])
    for part, sel in zip(("head", "rest"), parts):
        ref_err = ref[part] if isinstance(ref, dict) else errors(ref, exact, x, sel)
        tol, err = tolerance(ref_err), errors(got, exact, x, sel)
        ratios = {k: err[k] / tol[k] for k in err}
        print(f"{label} [{part}]: " + ", ".join(f"{k} {err[k]:.1e} / {tol[k]:.1e}" for k in err))
        worst = max(worst, max(ratios.values()))
        assert max(ratios.values()) <= 1.0, (label, part, err, tol)
    return worst


def pick(out):
    """(p_m_vecs, p_v_logdets, p_quads, nats) of a five-output tuple of ``block_form`` / ``row_loop`` / ``ld_row_loop``."""
    return out[0], out[2], out[3], out[4]


FIXTURES = [f"mvn_seq_d{D}_{kind}.npz" for D in (1, 3, 17) for kind in ("default", "diffuse", "posterior")]


def fixture_parts(g):
    """(x, start state as (m, kappa, nu, w_inv), long-double traces, the reference's recorded errors) of a fixture of
    tests/golden/make_golden_mvn_seq.py."""
    start = (g["start_m_vec"], float(g["start_kappa"]), float(g["start_nu"]), g["start_w_mat_inv"])
    exact = [g["exact_" + k] for k in NAMES]
    ref = {part: dict(zip(NAMES, g["ref_vs_exact_" + part])) for part in ("head", "rest")}
    return g["x"], start, exact, ref


def state_of(start):
    m, kappa, nu, w_inv = start
    return start_state(w_inv, m, kappa, nu)


# ---- the seam ----------------------------------------------------------------------------------------------------------------
class CpuMvnSeqPass:
    def __init__(self, D, blocks_per_pass=None):
        self.D = D
        self.device = torch.device("cpu")
        self.blocks_per_pass = blocks_per_pass
        self.launch_info = "cpu stand-in"

    def adopt(self, a):
        from bayesml_amd._regression import adopt_tensor
        return adopt_tensor(a, self.device)

    def run(self, x, start, want, chunk_bytes=None):
        assert x.dim() == 2 and x.shape[1] == self.D and x.dtype in (torch.float32, torch.float64)
        self.last_dtype, self.last_want = x.dtype, tuple(want)
        means, _nus, logdets, quads, nats = block_form(x.to(torch.float64).numpy(), np.asarray(start, dtype=np.float64),
                                                       self.blocks_per_pass)
        full = dict(means=means, logdet=logdets, quad=quads, nats=nats)
        return {k: torch.from_numpy(full[k]) for k in want}

    def close(self):
        pass


def stand_ins(m):
    from fake_engine import CpuDataPass
    m._data_pass_factory = CpuDataPass
    m._mvnseq_pass_factory = CpuMvnSeqPass
    return m


HN = ("hn_m_vec", "hn_kappa", "hn_nu", "hn_w_mat", "hn_w_mat_inv")


def model_at(D, start, device=None):
    """A LearnModel at the state ``start`` = (m, kappa, nu, w_inv): on the stand-ins without a device."""
    from bayesml_amd import multivariate_normal as mvn
    m = mvn.LearnModel(D, device=device)
    if device is None:
        stand_ins(m)
    if start is not None:
        mv, kappa, nu, w_inv = start
        m.set_hn_params(np.asarray(mv, dtype=np.float64), float(kappa), float(nu), np.linalg.inv(w_inv))
        m.hn_w_mat_inv[:] = w_inv           # the stored bits, not the inverse of their inverse
        m.calc_pred_dist()
    return m


def hn_equal(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in HN)


# ---- the models on the device (the GPU tests' helpers) ----------------------------------------------------------------------
def dev():
    return torch.device("cuda", 0)


def model(D, start=None):
    return model_at(D, start, device=dev())


def default_start(D):
    return (np.zeros(D), 1.0, float(D), np.eye(D))


def outputs(m, nats):
    return (m.p_m_vecs, m.p_v_logdets, m.p_quads, nats)


def sweep(label, D, ns, x, start, rows=None, make_model=None):
    """Every n of ``ns`` is a call on the first n rows; the loops run once, on the longest: prediction i does not depend on
    the rows after i.  ``rows``: the rows the long-double loop predicts and the comparison looks at (all if None).
    ``make_model``: (D, start) -> a model at that state; the device's ``model`` if None, ``model_at`` for the CPU stand-in."""
    make = model if make_model is None else make_model
    exact = pick(ld_row_loop(x, *start, rows=rows))
    ref = pick(row_loop(x, *start, rows=rows))
    worst = 0.0
    for n in ns:
        m = make(D, start)
        means, nats = m.pred_and_update_sequence(x[:n], code_length=True)
        got = outputs(m, nats)
        assert means.shape == (n, D) and all(a.shape == (n,) for a in got[1:]) and m.p_nus.shape == (n,)
        assert np.array_equal(m.p_nus, start[2] + np.arange(n) - D + 1)
        sub = None if rows is None else [i for i in rows if i < n]
        worst = max(worst, check(f"{label} n = {n}", got, [e[:n] for e in exact], [r[:n] for r in ref], x[:n], D, rows=sub))
        u = make(D, start).update_posterior(x[:n])
        assert hn_equal(m, u)
        u.calc_pred_dist()
        assert np.array_equal(m.p_m_vec, u.p_m_vec) and m.p_nu == u.p_nu and np.array_equal(m.p_v_mat, u.p_v_mat)
    print(f"{label}: worst error / tolerance {worst:.2f}")
    return worst


def second_call(label, D, x, start, n1, make_model=None):
    """Rows [0, n1) in one call and the rest in a second on the same model: the second call's pivot is its own row 0, and
    its start is whatever the first left.  The oracle starts from the model's own hn_* after the first call; hn_* after both
    and the next-point predictive are update_posterior's on the two pieces."""
    make = model if make_model is None else make_model
    m = make(D, start)
    m.pred_and_update_sequence(x[:n1])
    mid = (m.hn_m_vec.copy(), float(m.hn_kappa), float(m.hn_nu), m.hn_w_mat_inv.copy())
    x2 = x[n1:]
    n2 = len(x2)
    means, nats = m.pred_and_update_sequence(x2, code_length=True)
    got = outputs(m, nats)
    assert means.shape == (n2, D) and all(a.shape == (n2,) for a in got[1:])
    assert np.array_equal(m.p_nus, mid[2] + np.arange(n2) - D + 1)
    worst = check(label, got, pick(ld_row_loop(x2, *mid)), pick(row_loop(x2, *mid)), x2, D)
    u = make(D, start).update_posterior(x[:n1]).update_posterior(x2)
    assert hn_equal(m, u)
    u.calc_pred_dist()
    assert np.array_equal(m.p_m_vec, u.p_m_vec) and m.p_nu == u.p_nu and np.array_equal(m.p_v_mat, u.p_v_mat)
    print(f"{label}: worst error / tolerance {worst:.2f}")
    return worst


def synth(D, n, seed, loc=0.7, spread=1.0):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    return loc + spread * (rng.standard_normal((n, D)) @ mix.T)


def budget_for(D, blocks):
    """chunk_bytes that makes a pass hold so many blocks."""
    from bayesml_amd import _mvnseq
    return 8 * _mvnseq.work_slots(D, blocks)
