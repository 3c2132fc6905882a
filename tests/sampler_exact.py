"""The exact oracle and the derived bounds of the device samplers (csrc/sample.hip; TEST INFRASTRUCTURE, needs no GPU).

Oracle.  The raw 64-bit Philox4x64-10 integers are ``oracle/sampler_oracle.raw_blocks`` (NumPy's generator, pinned to the
Random123 known answers by tests/test_samplers.py).  From a block (r0, r1, r2, r3), with m = r >> 11,

    e = sqrt(-2 ln(1 - m0 2^-53)) (cos, sin)(2 pi m1 2^-53)          (and the same from (r2, r3))

is evaluated in mpmath at 60 digits (``cospi`` / ``sinpi``: no rounded pi enters) and kept as a ``np.longdouble`` with a 64-bit
significand, relative error <= 2^-64.  The emission x_j = mu_j + sum_{i >= j} e_i A_ij is then summed in ``np.longdouble``
from those normals and from the binary64 mu and A HANDED TO THE KERNEL, taken as exact: the error of the factorisation
that produced A is not the sampler's (tests/test_gpu_kside*.py own it).

Bound.  u = 2^-53 is the unit roundoff of binary64; an error of k ULP is a relative error of at most 2 k u.

  One device normal.  u0 = 1 - m0 2^-53 and 2 m1 2^-53 are exact, and so is -2 * log(u0).
      log        <= 1 ULP   relative 2 u; the square root halves a relative error of its argument:      1 u
      sqrt       <= 1 ULP                                                                               2 u
      sincospi   <= 2 ULP   each of the two results                                                     4 u
      rad * cs, rad * sn    one rounding                                                                1 u
                                                                                                c_e  =  8
  so |e_dev - e| <= c_e u |e| to first order.  The ULP figures are ASSUMED: they are the ones the public HIP math API
  documentation ("HIP math API", double precision floating-point functions: log 1, sqrt 1, sincospi 2) lists; that
  document is not part of the ROCm installation this suite was written on.  tests/test_gpu_sampler_edges.py measures the
  device's normals against them (profiles/sampler_tests.md).  m0 = 0 gives e = 0 exactly on both sides.

  One emission entry.  The grouped kernel runs one chain of D - j fused multiply-adds from mu_j, the plain kernel two
  chains of half the length and one addition: at most D - j + 1 roundings, each of a partial sum that is at most
  M_j = |mu_j| + sum_{i >= j} |e_i| |A_ij| in magnitude, and the perturbed normals move the sum by at most c_e u (M_j - |mu_j|):

      B_j = ((D - j + 2) + c_e) u M_j  +  (D + 2) 2^-64 M_j             (j counted from 0)

  The last term is the long-double reference's own error (2^-64 per normal, per product, per addition).  Tests allow
  2 B_j; the factor 2 covers the second-order terms and is the only margin.  Nothing in B_j comes from what the code
  under test returns.  ``float32`` output is ``(float)`` of the binary64 sum by the kernel's code, so it is compared bit
  for bit with the rounded binary64 output, not with a tolerance.

Host bound.  The float64 restatement ``sampler_oracle.normals`` does not meet c_e: it forms the angle as fl(fl(2 pi) f),
which is off by up to (0.35 + 1) u of an angle below 2 pi (fl(pi) is 0.35 u off, the product rounds once), 8.5 u ABSOLUTE,
so its cosine and sine are off by 8.5 u of the radius however small they are (measured: relative errors of 5e4 u where
|cos| is 1e-3).  That is a property of the restatement, not of the kernel, which calls ``sincospi`` on the exact 2 f.  The
CPU tests therefore hold the restatement to

    B_j(host) = ((D - j + 2) + c_h) u M_j + 8.5 u sum_{i >= j} rad_i |A_ij| + (D + 2) 2^-64 M_j,      c_h = 14,

with rad_i the Box-Muller radius behind e_i and c_h the same sum as c_e with 4 ULP ASSUMED for NumPy's log, cos and sin
(the accuracy its SIMD loops are built to) and a correctly rounded sqrt: 4 + 1 + 8 + 1.  NumPy's float64 SUM of the
exact normals rounded to float64 is held to B_j itself (the rounding of a normal is 1 u of the c_e = 8).

Chain.  ``chain_is_the_recursion`` checks z_0 = F_pi^-1(u_0) and z_t = F_{z_{t-1}}^-1(u_t) for every t >= 1 with the host's
uniforms; by induction on t that is equality with the sequential recursion, at O(T) NumPy cost.  ``chunk_maps`` restates
``chain_maps_kernel`` so that a chain case can assert that its chunk maps do NOT coalesce: only then does the state carried
across chunk borders decide anything; ``group_maps`` restates ``chain_compose_kernel`` for the same statement about the state
carried from group to group, which needs chains that do not forget their start within 65536 steps.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import sampler_oracle as so

U = 2.0 ** -53
C_E = 8.0                     # relative error of one device normal in units of u (module docstring)
C_H, ANGLE_H = 14.0, 8.5      # the float64 restatement's: relative, and absolute in units of u times the radius
CHUNK, GROUP = 256, 256       # csrc/sample.hip: kChunk, kGroup
DPS = 60

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit significand here: the emission oracle needs one"
LD = np.longdouble
LD_EPS = float(2.0 ** -64)


def _mp():
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = DPS
    return mp


def _to_ld(v) -> LD:
    """An mpf as hi + lo in long double (both parts are binary64, their sum carries 64 bits)."""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


@functools.lru_cache(maxsize=64)
def _normals_cached(seed: int, row0: int, n: int, D: int):
    mp = _mp()
    nb = (D + 3) // 4
    raw = so.raw_blocks(seed, 1, row0 * nb, n * nb)
    m = (raw >> np.uint64(11)).astype(object)               # exact Python integers
    out = np.zeros((n * nb, 4), dtype=LD)
    radius = np.zeros((n * nb, 4))
    two53 = mp.mpf(2) ** 53
    for b in range(n * nb):
        for h in (0, 1):
            m0, m1 = int(m[b, 2 * h]), int(m[b, 2 * h + 1])
            if m0 == 0:
                continue                                      # ln 1 = 0: both normals are exactly 0
            rad = mp.sqrt(-2 * mp.log(1 - mp.mpf(m0) / two53))
            ang = 2 * mp.mpf(m1) / two53
            out[b, 2 * h] = _to_ld(rad * mp.cospi(ang))
            out[b, 2 * h + 1] = _to_ld(rad * mp.sinpi(ang))
            radius[b, 2 * h] = radius[b, 2 * h + 1] = float(rad) * (1.0 + 2.0 ** -52)
    out, radius = out.reshape(n, 4 * nb)[:, :D], radius.reshape(n, 4 * nb)[:, :D]
    out.setflags(write=False)
    radius.setflags(write=False)
    return out, radius


def normals(seed: int, row0: int, n: int, D: int) -> np.ndarray:
    """e [n, D] in long double, each within 2^-64 relative of the exact Box-Muller normal of the stream."""
    return _normals_cached(int(seed), int(row0), int(n), int(D))[0]


def radii(seed: int, row0: int, n: int, D: int) -> np.ndarray:
    """rad [n, D]: the Box-Muller radius behind each normal, rounded up (float64)."""
    return _normals_cached(int(seed), int(row0), int(n), int(D))[1]


def normal_ratio(got, seed: int, row0: int = 0) -> float:
    """max |got - e| / (c_e u |e|) over the array (0 where both are exactly 0): a correct device stays below 2."""
    got = np.asarray(got, dtype=np.float64)
    e = normals(seed, row0, got.shape[0], got.shape[1])
    err = np.abs(got.astype(LD) - e)
    den = (C_E * U + LD_EPS) * np.abs(e)
    assert np.all(err[den == 0] == 0), "a normal that is exactly 0 was drawn as something else"
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), 0)))


class Emissions:
    """x (long double), M, B and B_host [n, D] of one call: ``z`` [n] classes, ``mu`` [K, D] and ``a`` [K, D, D] as handed
    over."""

    def __init__(self, z, mu, a, seed: int, row0: int = 0):
        z = np.asarray(z, dtype=np.int64)
        mu, a = np.asarray(mu, dtype=np.float64), np.asarray(a, dtype=np.float64)
        n, (K, D) = z.shape[0], mu.shape
        assert a.shape == (K, D, D) and (n == 0 or (z.min() >= 0 and z.max() < K))
        e, rad = normals(seed, row0, n, D), radii(seed, row0, n, D)
        self.x = np.empty((n, D), dtype=LD)
        self.M = np.empty((n, D), dtype=np.float64)
        R = np.empty((n, D), dtype=np.float64)
        for k in np.unique(z):
            rows = z == k
            ak = np.tril(a[k]).astype(LD)                     # the kernels read i >= j only
            self.x[rows] = mu[k].astype(LD) + e[rows] @ ak
            self.M[rows] = (np.abs(mu[k]).astype(LD) + np.abs(e[rows]) @ np.abs(ak)).astype(np.float64)
            R[rows] = rad[rows] @ np.abs(np.tril(a[k]))
        terms = D - np.arange(D) + 2.0
        self.B = ((terms + C_E) * U + (D + 2) * LD_EPS) * self.M
        self.B_host = ((terms + C_H) * U + (D + 2) * LD_EPS) * self.M + ANGLE_H * U * R
        self.e64 = e.astype(np.float64)                                       # the exact normals, rounded once
        self.old_tol = 2e-13 * (1.0 + np.abs(self.x.astype(np.float64)))      # tests/test_samplers.py: EPS_TOL

    def error(self, got) -> np.ndarray:
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == self.x.shape and np.all(np.isfinite(got)), "shape or a non-finite value"
        return np.abs(got.astype(LD) - self.x).astype(np.float64)

    def ratio(self, got, host: bool = False) -> float:
        """max |got - x| / B (entries with B = 0 must be exact): the tests allow 2.  ``host``: against B(host)."""
        err, B = self.error(got), self.B_host if host else self.B
        assert np.all(err[B == 0] == 0)
        return float(np.max(np.where(B > 0, err / np.where(B > 0, B, 1), 0), initial=0.0))

    def old_ratio(self, got) -> float:
        """max |got - x| / (2e-13 (1 + |x|)): the hand-picked tolerance of tests/test_samplers.py, for comparison."""
        return float(np.max(self.error(got) / self.old_tol, initial=0.0))


# ---- Markov chain ------------------------------------------------------------------------------------------------------

def _inverse_by_state(cum, prev, u):
    """F_{prev_i}^-1(u_i) for vectors: the number of entries of cum[prev_i, :-1] that are <= u_i."""
    out = np.empty(prev.shape[0], dtype=np.int64)
    for s in np.unique(prev):
        at = prev == s
        out[at] = np.searchsorted(cum[s, :-1], u[at], side="right")
    return out


def chain_first_mismatch(z, pi, a, seed: int, slab: int = 1 << 22) -> int:
    """The first t at which ``z`` is not one step of the recursion from z[t - 1] (t = 0: from pi); -1 if there is none.
    An entry outside [0, K) counts as a mismatch at its position."""
    z = np.asarray(z)
    pi, a = np.asarray(pi, dtype=np.float64), np.asarray(a, dtype=np.float64)
    K, T = pi.shape[0], z.shape[0]
    if T == 0:
        return -1
    bad = np.flatnonzero((z < 0) | (z >= K))
    limit = int(bad[0]) if bad.size else T
    cp, ca = np.cumsum(pi), np.cumsum(a, axis=1)
    for t0 in range(0, limit, slab):
        m = min(slab, limit - t0)
        u = so.latent_uniforms(seed, t0, m)
        want = np.empty(m, dtype=np.int64)
        lo = 0
        if t0 == 0:
            want[0] = np.searchsorted(cp[:-1], u[0], side="right")
            lo = 1
        want[lo:] = _inverse_by_state(ca, np.asarray(z[t0 + lo - 1:t0 + m - 1], dtype=np.int64), u[lo:])
        off = np.flatnonzero(want != z[t0:t0 + m])
        if off.size:
            return t0 + int(off[0])
    return limit if bad.size else -1


def chain_is_the_recursion(z, pi, a, seed: int) -> bool:
    return chain_first_mismatch(z, pi, a, seed) == -1


def chunk_maps(pi, a, seed: int, T: int, slab: int = 2048) -> np.ndarray:
    """maps [ceil(T / 256), K] of ``chain_maps_kernel``: the state after chunk c when it is entered in state s (the very
    first step draws from pi whatever s is).  Vectorised over chunks."""
    pi, a = np.asarray(pi, dtype=np.float64), np.asarray(a, dtype=np.float64)
    K = pi.shape[0]
    cp, ca = np.cumsum(pi), np.cumsum(a, axis=1)
    n_chunks = (T + CHUNK - 1) // CHUNK
    maps = np.empty((n_chunks, K), dtype=np.int64)
    small = np.int16 if K < 2 ** 15 else np.int64
    for c0 in range(0, n_chunks, slab):
        c1 = min(n_chunks, c0 + slab)
        t0, t1 = c0 * CHUNK, min(T, c1 * CHUNK)
        u = np.full((c1 - c0) * CHUNK, -1.0)
        u[:t1 - t0] = so.latent_uniforms(seed, t0, t1 - t0)
        u = u.reshape(c1 - c0, CHUNK)
        step = np.empty((c1 - c0, CHUNK, K), dtype=small)      # step[c, t, s]: where state s goes at step t of chunk c
        for s in range(K):
            step[:, :, s] = np.where(u >= 0, np.searchsorted(ca[s, :-1], u, side="right"), s)     # past T: stay
        if c0 == 0:
            step[0, 0, :] = np.searchsorted(cp[:-1], u[0, 0], side="right")
        cur = np.broadcast_to(np.arange(K), (c1 - c0, K)).copy()
        rows = np.arange(c1 - c0)[:, None]
        for t in range(CHUNK):
            cur = step[rows, t, cur].astype(np.int64)
        maps[c0:c1] = cur
    return maps


def nonconstant_maps(maps) -> int:
    """How many chunk maps take more than one value (the first chunk's never does: it starts from pi)."""
    return int(np.sum(maps.max(axis=1) != maps.min(axis=1)))


def group_maps(maps) -> np.ndarray:
    """gmaps [ceil(n_chunks / 256), K] of ``chain_compose_kernel``: a group's chunk maps composed in time order."""
    n_chunks, K = maps.shape
    n_groups = (n_chunks + GROUP - 1) // GROUP
    padded = np.broadcast_to(np.arange(K), (n_groups * GROUP, K)).copy()          # past the last chunk: the identity
    padded[:n_chunks] = maps
    padded = padded.reshape(n_groups, GROUP, K)
    cur = np.broadcast_to(np.arange(K), (n_groups, K)).copy()
    rows = np.arange(n_groups)[:, None]
    for c in range(GROUP):
        cur = padded[rows, c, cur]
    return cur


def chain_precondition(pi, a, seed: int, T: int) -> tuple:
    """(non-constant chunk maps, chunks after the first).  A chain case needs at least half of the latter non-constant."""
    maps = chunk_maps(pi, a, seed, T)
    return nonconstant_maps(maps[1:]), maps.shape[0] - 1


def recursion_from(pi, a, seed: int, t0: int, T: int, state: int) -> np.ndarray:
    """z[t0 .. T) of the sequential recursion entered at step t0 in ``state`` (t0 = 0: the first step draws from pi)."""
    u = so.latent_uniforms(seed, t0, T - t0)
    cp, ca = np.cumsum(pi), np.cumsum(np.asarray(a, dtype=np.float64), axis=1)
    out = np.empty(T - t0, dtype=np.int64)
    s = int(state)
    for i in range(T - t0):
        s = int(np.searchsorted(cp[:-1] if t0 + i == 0 else ca[s, :-1], u[i], side="right"))
        out[i] = s
    return out


def chain_from_maps(pi, a, seed: int, T: int, maps) -> np.ndarray:
    """The device's plan on the host: entry states by composing ``maps`` chunk after chunk, then every chunk replayed from
    its entry state.  With the true ``chunk_maps`` this is the recursion; the CPU tests hand it damaged maps."""
    z = np.empty(T, dtype=np.int64)
    cur = 0
    for c in range(maps.shape[0]):
        t0 = c * CHUNK
        z[t0:t0 + CHUNK] = recursion_from(pi, a, seed, t0, min(T, t0 + CHUNK), cur)
        cur = int(maps[c, cur])
    return z
