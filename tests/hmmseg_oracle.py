"""The exact oracle and the derived bound of the forward-backward pass over many sequences (csrc/hmmseg_kernels.h).

Oracle.  ``exact(ln_rho, pi, a, off)`` takes the ln rho array the engine holds after ``estep`` and the pi~, A~ and ``off``
HANDED TO ``forward_backward_segments`` as exact binary64 values and evaluates, per segment and each segment on its own, in
mpmath at ``contexttree_oracle._mp()`` digits: rho'_t = exp(ln rho_t - max_k ln rho_tk), alpha_t, c'_t, beta_t, gamma_t, xi_t
for t past the segment's first row, ms = sum xi, g0, gl and sum (ln c'_t + max_t).  Zero entries of A~ (and of alpha) are
skipped.  So what is held to it are hmm_prep_kernel, the three hmmseg kernels, hmm_xi_sum_kernel, finish_pass and the two
ends kernels; the emission kernel is tested elsewhere.

Bound ("Fit from many sequences", *Error bound*).  eps = 2^-52; all bounds are on |ln(device / exact)|, the
relative error to first order:

    e_t   = max_k (|ln rho_tk - max_t| + 3) eps         the rounded subtraction, the device exponential
    h_t   = 2 e_t + 2 (K + 3) eps                       what one normalised step adds in the projective (Hilbert) metric, in
                                                        which it is non-expansive: a K-term dot product of non-negative terms
                                                        in any order, the product with rho', the renormalisation
    Hf_t  = sum of h over the segment's rows up to t,   Hb_t = sum of h over the segment's rows after t
    alpha_tk      Hf_t + (K + 1) eps                    (the sum of the device's alpha_t is 1 only to (K + 1) eps)
    gamma_tk      Hf_t + Hb_t + (K + 4) eps
    c'_t          Hf_{t-1} + e_t + (3 K + 2) eps
    xi_t[i, j]    Hf_{t-1} + Hb_t + 2 e_t + (2 K + 16) eps
    ms, g0, gl    the largest bound of their terms + (number of non-zero terms + 2) eps  (sums of non-negative terms in any
                  order: a zero term - padding, an empty slab or block - adds nothing)
    sum ln c      sum_t bound(c'_t) + 2 eps sum_t (|ln c'_t| + |max_t|) + T eps sum_t |ln c'_t + max_t|

The device is held to twice the bound (second-order terms), a binary64 implementation in any summation order to once.
Nothing in the bound comes from what the code under test returns.  The derivation assumes no underflow: ``guard`` is the
smallest non-zero product the recursions form, and the cases keep it far above the smallest normal number.

Small entries.  An entry whose exact value is 0 must be 0; one below ``TINY`` = 1e-290 is checked absolutely; ``small_share``
is the share of alpha and gamma entries under that rule.
"""
import numpy as np

import contexttree_oracle as cto

EPS = 2.0 ** -52
TINY = 1e-290


class Exact:
    """alpha, gamma [T, K], cprime [T], xi [T, K, K], ms [K, K], g0, gl [K] as floats (rounded once), their exact-zero masks
    ``z_*``, lnc (mpf), and the bounds b_alpha, b_gamma, b_c, b_xi [T], b_ms, b_g0, b_gl, b_lnc (floats)."""

    def _ratio(self, name, got, exact, zero, bound):
        """max |got - exact| / (exact * bound) over the entries at or above TINY; the zero and the small rule asserted."""
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == exact.shape and np.all(np.isfinite(got)), name
        assert np.all(got[zero] == 0.0), f"{name}: an entry that is exactly 0 is not 0 on the device"
        small = ~zero & (exact < TINY)
        assert np.all(np.abs(got[small] - exact[small]) <= TINY), f"{name}: an entry below {TINY} is off by more"
        live = ~zero & ~small
        if not live.any():
            return 0.0
        bound = np.broadcast_to(bound, exact.shape)
        # (exact was rounded to binary64 once: half an eps is added to the measured error, never taken off it)
        return float(np.max((np.abs(got[live] - exact[live]) / exact[live] + 0.5 * EPS) / bound[live]))

    def ratios(self, got):
        """{quantity: worst |error| / bound} of a result dict with alpha, gamma, cprime, xi, ms, g0, gl, lnc."""
        mp = cto._mp()
        r = dict(alpha=self._ratio("alpha", got["alpha"], self.alpha, self.z_alpha, self.b_alpha[:, None]),
                 gamma=self._ratio("gamma", got["gamma"], self.gamma, self.z_gamma, self.b_gamma[:, None]),
                 cprime=self._ratio("cprime", got["cprime"], self.cprime, np.zeros(len(self.cprime), dtype=bool), self.b_c),
                 xi=self._ratio("xi", got["xi"], self.xi, self.z_xi, self.b_xi[:, None, None]),
                 ms=self._ratio("ms", got["ms"], self.ms, self.z_ms, self.b_ms),
                 g0=self._ratio("g0", got["g0"], self.g0, self.z_g0, self.b_g0),
                 gl=self._ratio("gl", got["gl"], self.gl, self.z_gl, self.b_gl))
        r["lnc"] = float(abs(mp.mpf(float(got["lnc"])) - self.lnc)) / self.b_lnc
        return r


def _floats(rows, shape):
    """(binary64 array, exact-zero mask) of nested lists of mpf."""
    flat = np.array([float(v) for v in rows], dtype=np.float64).reshape(shape)
    zero = np.array([v == 0 for v in rows], dtype=bool).reshape(shape)
    return flat, zero


def exact(ln_rho, pi, a, off):
    mp = cto._mp()
    ln_rho, pi, a = (np.asarray(v, dtype=np.float64) for v in (ln_rho, pi, a))
    T, K = ln_rho.shape
    off = [int(v) for v in off]
    assert off[0] == 0 and off[-1] == T
    mx = ln_rho.max(axis=1)
    zero, one = mp.mpf(0), mp.mpf(1)
    pim = [mp.mpf(v) for v in pi]
    col = [[(i, mp.mpf(a[i, j])) for i in range(K) if a[i, j] != 0.0] for j in range(K)]      # column j of A~
    row = [[(j, mp.mpf(a[i, j])) for j in range(K) if a[i, j] != 0.0] for i in range(K)]      # row i
    d = np.zeros((T, K))
    alpha, gamma, cp, xi = [None] * T, [None] * T, [None] * T, [[zero] * (K * K) for _ in range(T)]
    ms, g0, gl, lnc = [zero] * (K * K), [zero] * K, [zero] * K, zero
    guard = np.inf

    def seen(values):
        nonlocal guard
        nz = [v for v in values if v != 0]
        if nz:
            guard = min(guard, float(min(nz)))

    n_first = 0
    for lo, hi in zip(off[:-1], off[1:]):
        if hi == lo:
            continue
        n_first += 1
        rho = []
        for t in range(lo, hi):
            dt = [mp.mpf(ln_rho[t, k]) - mp.mpf(mx[t]) for k in range(K)]
            d[t] = [float(v) for v in dt]
            rho.append([mp.exp(v) for v in dt])
        prev = None
        for t in range(lo, hi):
            r = rho[t - lo]
            if t == lo:
                v = [pim[k] * r[k] for k in range(K)]
            else:
                v = [r[k] * mp.fsum(prev[i] * aik for i, aik in col[k] if prev[i] != 0) for k in range(K)]
            seen(v)
            cp[t] = mp.fsum(v)
            assert cp[t] > 0, "a row's c' is 0: the case is not one the pass is asked about"
            prev = alpha[t] = [vk / cp[t] for vk in v]
            lnc += mp.log(cp[t]) + mp.mpf(mx[t])
        beta = [one] * K                                              # scaled like the reference's: gamma = alpha o beta
        for t in range(hi - 1, lo - 1, -1):
            gamma[t] = [alpha[t][k] * beta[k] for k in range(K)]
            if t == lo:
                break
            r = rho[t - lo]
            y = [r[j] * beta[j] for j in range(K)]
            tot = mp.fsum(beta)
            seen([v / tot for v in y])                                # (the device carries beta at sum 1)
            w = [v / cp[t] for v in y]
            x_t = xi[t]
            for i in range(K):
                ai = alpha[t - 1][i]
                if ai != 0:
                    for j, aij in row[i]:
                        x_t[i * K + j] = ai * aij * w[j]
                        ms[i * K + j] += x_t[i * K + j]
            beta = [mp.fsum(aij * w[j] for j, aij in row[i]) for i in range(K)]
        g0 = [u + v for u, v in zip(g0, gamma[lo])]
        gl = [u + v for u, v in zip(gl, gamma[hi - 1])]

    o = Exact()
    o.K, o.T, o.guard, o.d_min, o.lnc, o.n_first = K, T, guard, float(d.min()) if T else 0.0, lnc, n_first
    o.alpha, o.z_alpha = _floats([v for t in range(T) for v in alpha[t]], (T, K))
    o.gamma, o.z_gamma = _floats([v for t in range(T) for v in gamma[t]], (T, K))
    o.cprime = np.array([float(v) for v in cp])
    o.xi, o.z_xi = _floats([v for t in range(T) for v in xi[t]], (T, K, K))
    o.ms, o.z_ms = _floats(ms, (K, K))
    o.g0, o.z_g0 = _floats(g0, (K,))
    o.gl, o.z_gl = _floats(gl, (K,))
    both = np.concatenate([o.alpha[~o.z_alpha], o.gamma[~o.z_gamma]])
    o.small_share = float(np.mean(both < TINY)) if both.size else 0.0

    # ---- the bound (floats; every quantity in it is a size, not a difference) ----
    e = (np.abs(d).max(axis=1) + 3.0) * EPS
    h = 2.0 * e + 2.0 * (K + 3) * EPS
    hf, hf_prev, hb = np.zeros(T), np.zeros(T), np.zeros(T)
    for lo, hi in zip(off[:-1], off[1:]):
        if hi > lo:
            c = np.cumsum(h[lo:hi])
            hf[lo:hi], hf_prev[lo:hi], hb[lo:hi] = c, c - h[lo:hi], c[-1] - c
    o.e, o.h, o.hf, o.hb = e, h, hf, hb
    o.b_alpha = hf + (K + 1) * EPS
    o.b_gamma = hf + hb + (K + 4) * EPS
    o.b_c = hf_prev + e + (3 * K + 2) * EPS
    o.b_xi = hf_prev + hb + 2.0 * e + (2 * K + 16) * EPS
    inner = np.ones(T, dtype=bool)
    inner[[v for v, w in zip(off[:-1], off[1:]) if w > v]] = False          # rows past their segment's first
    firsts = np.array([v for v, w in zip(off[:-1], off[1:]) if w > v], dtype=np.int64)
    lasts = np.array([w - 1 for v, w in zip(off[:-1], off[1:]) if w > v], dtype=np.int64)
    o.b_ms = (o.b_xi[inner].max() if inner.any() else 0.0) + (int(inner.sum()) + 2) * EPS
    o.b_g0 = o.b_gamma[firsts].max() + (n_first + 2) * EPS
    o.b_gl = o.b_gamma[lasts].max() + (n_first + 2) * EPS
    ln_c = np.array([float(mp.log(v)) for v in cp])
    o.b_lnc = float(o.b_c.sum() + 2.0 * EPS * (np.abs(ln_c) + np.abs(mx)).sum() + T * EPS * np.abs(ln_c + mx).sum())
    return o


def binary64(ln_rho, pi, a, off):
    """The same quantities by the reference's scaled recursions (oracle.hmm_vb_oracle.forward_backward) in binary64, each
    segment on its own: a legitimate implementation the bound must leave room for."""
    from oracle import hmm_vb_oracle as orc
    ln_rho = np.asarray(ln_rho, dtype=np.float64)
    T, K = ln_rho.shape
    mx = ln_rho.max(axis=1)
    rho = np.exp(ln_rho - mx[:, None])
    r = dict(alpha=np.zeros((T, K)), gamma=np.zeros((T, K)), cprime=np.ones(T), xi=np.zeros((T, K, K)), ms=np.zeros((K, K)),
             g0=np.zeros(K), gl=np.zeros(K))
    for lo, hi in zip(off[:-1], off[1:]):
        if hi > lo:
            al, be, c = orc.forward_backward(rho[lo:hi], pi, a)
            r["alpha"][lo:hi], r["gamma"][lo:hi], r["cprime"][lo:hi] = al, al * be, c
            r["xi"][lo + 1:hi] = al[:-1, :, None] * a[None] * (rho[lo + 1:hi] * be[1:] / c[1:, None])[:, None, :]
            r["g0"] += r["gamma"][lo]
            r["gl"] += r["gamma"][hi - 1]
    r["ms"] = r["xi"].sum(axis=0)
    r["lnc"] = float((np.log(r["cprime"]) + mx).sum())
    return r
