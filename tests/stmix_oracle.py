"""The exact oracle, the derived bound and the CPU stand-in of the Student-t mixture log-density (include/stmix.h).

Oracle.  ``exact(...)`` evaluates ln p_i, t_ik and r_ik = exp(t_ik - ln p_i) from the U_k, mu_k, nu_k, pi_k and x HANDED TO
THE ENGINE, binary64 values taken as exact, so the factorisation that produced U_k is not charged to the kernel.  The
quadratic forms q_ik = ||U_k (x_i - mu_k)||^2 are formed in exact integer arithmetic (every binary64 value is an integer
times a power of two; Python integers do not round), everything after them - lnGamma, log1p, the log-sum-exp - in mpmath
at the project's ``contexttree_oracle._mp()`` digits.

Bound.  With eps = 2^-52, xc = x_i - p, d = mu_k - p, y = U_k (x_i - mu_k):

    S_j  = sum_l |U_jl| (|xc_l| + |d_l|)                        the sizes the row sums of y_j add up
    dq   = 2 (D + 2) eps sum_j |y_j| S_j + (D + 2) eps q         q = sum y_j^2 from D + 2 roundings per y_j and per sum
    C_k  = |ln pi_k| + |lnG(a) - lnG(nu/2)| + |(D/2) ln(nu pi)| + sum_j |ln U_jj|
    B_ik = a_k dq / (nu_k + q) + 4 eps (C_k + a_k log1p(q / nu_k))   d/dq [a log1p(q / nu)] = a / (nu + q)
    B_i  = sum_k r_ik B_ik + 4 eps (1 + |ln p_i|)                d ln p / d t_k = r_ik

The GPU tests assert |ln p_i(engine) - ln p_i(exact)| <= 2 B_i (the 2 covers second-order terms), the CPU restatement is
held inside B_i itself.  Nothing in the bound comes from what the code under test returns.

Stand-in.  ``StandIn`` restates the kernels' form in NumPy - the pivot, the image's bias -U_k (mu_k - p), y = U_k xc + bias,
the online log-sum-exp in k order with the first arg-max - behind the models' ``_stmix_pass_factory`` seam.
"""
import numpy as np
import torch

import contexttree_oracle as orc

EPS = float(np.finfo(np.float64).eps)


# ---- exact quadratic forms -------------------------------------------------------------------------------------------------
def _ints(a):
    """(object array of Python ints, e) with a == ints * 2**-e exactly."""
    flat = [float(v).as_integer_ratio() for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    e = max(den.bit_length() - 1 for _, den in flat)
    out = np.empty(len(flat), dtype=object)
    for i, (num, den) in enumerate(flat):
        out[i] = num << (e - (den.bit_length() - 1))
    return out.reshape(np.shape(a)), e


def exact_y(u, mu, x):
    """y[k, j, i] = (U_k (x_i - mu_k))_j as exact integers, and the exponent e with y = ints * 2**-e."""
    K, D, _ = u.shape
    both, ex = _ints(np.concatenate([np.asarray(x, dtype=np.float64), mu]))
    xi, mi = both[:len(x)], both[len(x):]
    ui, eu = _ints(np.tril(u))
    y = np.empty((K, D, len(x)), dtype=object)
    for k in range(K):
        y[k] = np.dot(ui[k], (xi - mi[k][None, :]).T)
    return y, eu + ex


class Exact:
    """ln p (mpf list ``lnp_mp``, floats ``lnp``), t, r, q [N, K] floats, the arg-max ``z`` and the bounds B [N], B_ik [N, K]."""

    def ratio(self, got):
        """max_i |got_i - ln p_i| / B_i with the difference taken in mpmath, and the row it is reached at."""
        mp = orc._mp()
        err = np.array([float(abs(mp.mpf(float(g)) - e)) for g, e in zip(np.asarray(got), self.lnp_mp)])
        assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), "the engine returned a non-finite ln p"
        r = err / self.B
        return float(r.max()), int(r.argmax())

    def z_decided(self):
        """Rows whose two largest t differ by more than 2 (B_ik + B_ik'): there the engine's arg-max must be ``z``."""
        if self.t.shape[1] == 1:
            return np.ones(len(self.t), dtype=bool)
        order = np.argsort(-self.t, axis=1, kind="stable")
        rows = np.arange(len(self.t))
        k1, k2 = order[:, 0], order[:, 1]
        return self.t[rows, k1] - self.t[rows, k2] > 2.0 * (self.Bik[rows, k1] + self.Bik[rows, k2])


def exact(u, mu, nu, pi, pivot, x):
    mp = orc._mp()
    u, mu, nu, pi = (np.asarray(a, dtype=np.float64) for a in (u, mu, nu, pi))
    x = np.asarray(x)
    xf = x.astype(np.float64)                     # (widening is exact)
    pivot = np.asarray(pivot, dtype=np.float64)
    K, D, _ = u.shape
    N = len(xf)
    y_int, e = exact_y(u, mu, xf)
    q_int = (y_int * y_int).sum(axis=1)           # [K, N] exact
    scale = mp.mpf(2) ** (-2 * e)
    den = 1 << e
    y = np.frompyfunc(lambda v: v / den, 1, 1)(y_int).astype(np.float64)      # (int / int: correctly rounded)
    # the constants
    c_mp, C = [], np.zeros(K)
    for k in range(K):
        a, hv = (mp.mpf(nu[k]) + D) / 2, mp.mpf(nu[k]) / 2
        terms = [mp.log(mp.mpf(pi[k])), mp.loggamma(a) - mp.loggamma(hv), -(mp.mpf(D) / 2) * mp.log(mp.mpf(nu[k]) * mp.pi)]
        diag = [mp.log(mp.mpf(u[k, j, j])) for j in range(D)]
        c_mp.append(mp.fsum(terms) + mp.fsum(diag))
        C[k] = float(sum(abs(v) for v in terms) + sum(abs(v) for v in diag))
    o = Exact()
    o.lnp_mp, t, r, q, L = [], np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K))
    for i in range(N):
        ti = []
        for k in range(K):
            qk = mp.mpf(int(q_int[k, i])) * scale
            lk = mp.log1p(qk / mp.mpf(nu[k]))
            ti.append(c_mp[k] - (mp.mpf(nu[k]) + D) / 2 * lk)
            q[i, k], L[i, k] = float(qk), float(lk)
        top = max(ti)
        lnp = top + mp.log(mp.fsum(mp.exp(v - top) for v in ti))
        o.lnp_mp.append(lnp)
        t[i] = [float(v) for v in ti]
        r[i] = [float(mp.exp(v - lnp)) for v in ti]
    # the bound (floats; every quantity in it is a size, not a difference)
    a = 0.5 * (nu + D)
    xc, d = np.abs(xf - pivot), np.abs(mu - pivot)
    S = np.einsum("kjl,il->ikj", np.abs(np.tril(u)), xc) + np.einsum("kjl,kl->kj", np.abs(np.tril(u)), d)[None]     # [N, K, D]
    dq = 2 * (D + 2) * EPS * np.einsum("kji,ikj->ik", np.abs(y), S) + (D + 2) * EPS * q
    o.Bik = a[None] * dq / (nu[None] + q) + 4 * EPS * (C[None] + a[None] * L)
    o.lnp = np.array([float(v) for v in o.lnp_mp])
    o.B = (r * o.Bik).sum(axis=1) + 4 * EPS * (1 + np.abs(o.lnp))
    o.t, o.r, o.q, o.C = t, r, q, C
    o.z = np.argmax(t, axis=1)                    # (the first maximum)
    return o


def exact_from_precision(lam, mu, nu, pi, x):
    """(ln p [N] floats, cond [K]) from the precision matrices themselves (a model's ``p_lambda_mats``): q = (x - mu)^T Lambda
    (x - mu) in exact integers, ln det Lambda / 2 from an mpmath Cholesky, no factor of the engine's involved - for the
    model tests, whose engine factorises on its own."""
    mp = orc._mp()
    lam, mu, nu, pi = (np.asarray(a, dtype=np.float64) for a in (lam, mu, nu, pi))
    xf = np.asarray(x).astype(np.float64)
    K, D, _ = lam.shape
    both, ex = _ints(np.concatenate([xf, mu]))
    xi, mi = both[:len(xf)], both[len(xf):]
    li, el = _ints(lam)
    scale = mp.mpf(2) ** (-(2 * ex + el))
    c, q_int = [], []
    for k in range(K):
        chol = mp.cholesky(mp.matrix(lam[k].tolist()))
        half_logdet = mp.fsum(mp.log(chol[j, j]) for j in range(D))
        a, hv = (mp.mpf(nu[k]) + D) / 2, mp.mpf(nu[k]) / 2
        c.append(mp.log(mp.mpf(pi[k])) + mp.loggamma(a) - mp.loggamma(hv) - (mp.mpf(D) / 2) * mp.log(mp.mpf(nu[k]) * mp.pi)
                 + half_logdet)
        dv = xi - mi[k][None, :]
        q_int.append((np.dot(dv, li[k]) * dv).sum(axis=1))
    out = []
    for i in range(len(xf)):
        ti = [c[k] - (mp.mpf(nu[k]) + D) / 2 * mp.log1p(mp.mpf(int(q_int[k][i])) * scale / mp.mpf(nu[k])) for k in range(K)]
        top = max(ti)
        out.append(float(top + mp.log(mp.fsum(mp.exp(v - top) for v in ti))))
    return np.array(out), np.linalg.cond(lam)


def model_tolerance(D, cond, lnp):
    """For ``calc_pred_logpdf`` of a model against ``exact_from_precision``.  The model factorises hn_w_mats_inv while the
    oracle reads p_lambda_mats, the host's inverse of the same matrix: the two differ by the conditioning of that matrix
    times a few roundings per entry, which moves q and ln det relatively by about D eps cond; 64 of those, relative to the
    size of ln p (and never below the 64 eps (1 + |ln p|) this gives at cond = 1, D = 1)."""
    return 64 * D * EPS * np.max(cond) * (1.0 + np.abs(lnp))


# ---- the kernels' form in NumPy ----------------------------------------------------------------------------------------------
def restate(x, pi, mu, nu, u, pivot=None, c=None):
    """(ln p, z) by the kernels' operations in binary64 NumPy: rows centred about the pivot (row 0 of x by default) as they are
    widened, y = U_k xc + bias with bias = -U_k (mu_k - p), the online log-sum-exp in k order, the first arg-max."""
    from bayesml_amd import _stmix
    pi, mu, nu, u = (np.asarray(a, dtype=np.float64) for a in (pi, mu, nu, u))
    xf = np.asarray(x).astype(np.float64)
    p = xf[0].copy() if pivot is None else np.asarray(pivot, dtype=np.float64)
    K, D, _ = u.shape
    if c is None:
        c = _stmix.log_norm_consts(torch.from_numpy(pi), torch.from_numpy(nu), torch.from_numpy(u)).numpy()
    xc = xf - p
    M = np.full(len(xf), -np.inf)
    s = np.zeros(len(xf))
    z = np.zeros(len(xf), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            uk = np.tril(u[k])
            bias = -(uk @ (mu[k] - p))
            y = xc @ uk.T + bias
            q = (y * y).sum(axis=1)
            t = c[k] - 0.5 * (nu[k] + D) * np.log1p(q / nu[k])
            dlt = t - M
            e = np.where(t == -np.inf, 0.0, np.exp(-np.abs(dlt)))
            up = dlt > 0
            s = np.where(up, s * e + 1.0, s + e)
            z = np.where(up, k, z)
            M = np.where(up, t, M)
        return M + np.log(s), z


class StandIn:
    """``_stmix.StudentMixturePass`` on the CPU, for the models' ``_stmix_pass_factory`` seam."""
    calls = 0

    def __init__(self, K, D):
        self.K, self.D, self.device = K, D, torch.device("cpu")
        self.last = None

    def adopt(self, a):
        from bayesml_amd._regression import adopt_tensor
        return adopt_tensor(a, self.device)

    def run(self, x, pi, mu, nu, u, want_z, pivot=None):
        StandIn.calls += 1
        assert x.dtype in (torch.float32, torch.float64) and x.shape[1] == self.D and u.shape == (self.K, self.D, self.D)
        args = [t.detach().numpy() for t in (pi, mu, nu, u)]
        self.last = dict(pi=args[0], mu=args[1], nu=args[2], u=args[3], pivot=x[0].double().numpy().copy(), x=x.numpy())
        lnp, z = restate(x.numpy(), *args, pivot=pivot)
        return torch.from_numpy(lnp), (torch.from_numpy(z) if want_z else None)
