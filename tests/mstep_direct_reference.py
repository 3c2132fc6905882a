"""Long-double reference of the M-step's raw sums and the rounding bound they are held to (tests/test_gpu_mstep_direct.py).

The M-step accumulates, per component k and about a pivot p,
    ns_k = sum_t w_tk,  a_k = sum_t w_tk xc_t,  B_k = sum_t w_tk xc_t xc_t^T,  h_k = sum_t (a per-mode term),
with xc_t = (double)x_t - p rounded once to binary64 - the value the kernels form (or read from the centred copy).  Here
the same binary64 factors are multiplied and added in np.longdouble, next to the sum of the terms' absolute values, which
is the scale of the bound: both sides add the same binary64 products in another order, and the device rounds w xc once
before the MFMA, so every entry obeys
    |device - reference| <= (N + 8) 2^-53 sum_t |term_t|
per entry and per component (not per array: a component of weight 1e-40 is not hidden behind its neighbours)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
# (the bound assumes a reference far more precise than binary64: x87 extended or wider)
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than binary64 on this host: no reference for the M-step bound"


def centred(x, pivot):
    """(double)x - pivot, rounded once to binary64."""
    return np.asarray(x, dtype=np.float64) - np.asarray(pivot, dtype=np.float64)


def weighted_sums(x, pivot, w):
    """(value, scale) pairs of ns [K], a [K, D], B [K, D, D] for weights w [N, K] >= 0: long-double sums of the terms and of
    their absolute values."""
    xc = centred(x, pivot).astype(LD)
    xa = np.abs(xc)
    w = np.asarray(w, dtype=np.float64).astype(LD)
    assert float(w.min()) >= 0.0
    N, D = xc.shape
    K = w.shape[1]
    ns = w.sum(axis=0)
    a, a_abs = w.T @ xc, w.T @ xa
    B, B_abs = np.empty((K, D, D), dtype=LD), np.empty((K, D, D), dtype=LD)
    for k in range(K):
        wk = w[:, k][:, None]
        B[k] = (wk * xc).T @ xc
        B_abs[k] = (wk * xa).T @ xa
    return dict(ns=(ns, ns.copy()), a=(a, a_abs), B=(B, B_abs))


def h_hmm(gamma, ln_rho):
    """h_k = sum_t gamma_tk ln rho_tk over gamma > 0 (the kernels' guard), and its scale."""
    g = np.asarray(gamma, dtype=np.float64).astype(LD)
    lr = np.where(np.asarray(gamma) > 0.0, np.asarray(ln_rho, dtype=np.float64), 0.0).astype(LD)
    t = g * lr
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def h_loaded(r):
    """h_k = sum_{r > 0} r ln r, and its scale."""
    r = np.asarray(r, dtype=np.float64).astype(LD)
    t = np.zeros_like(r)
    pos = r > 0
    t[pos] = r[pos] * np.log(r[pos])
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def worst_ratio(device, value, scale, n_rows):
    """max over the entries of |device - value| / ((N + 8) 2^-53 scale); an entry of scale 0 must be exact (inf otherwise)."""
    err = np.abs(np.asarray(device, dtype=np.float64).astype(LD) - value)
    bound = LD(n_rows + 8) * LD(U) * scale
    ratio = np.zeros(err.shape, dtype=np.float64)
    nz = bound > 0
    ratio[nz] = (err[nz] / bound[nz]).astype(np.float64)
    ratio[~nz & (err > 0)] = np.inf
    return float(ratio.max()) if ratio.size else 0.0
