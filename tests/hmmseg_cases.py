"""The shapes of tests/test_gpu_hmmseg_edges.py and tests/test_hmmseg_oracle.py: batches of sequences at the branch edges of
csrc/hmmseg_kernels.h and of run_segments (csrc/hmm_capi.hip).  D = 2, float64 rows, the non-fused emission, one fixed pivot.

Exact-oracle cases (``EXACT``) stay at or below about 165 rows and K^2 T <= 3e5, so the mpmath recursion of
tests/hmmseg_oracle.py takes a few seconds at the most; the binary64 cases (``ONES``, ``REUSE``, ``ENDS``) have too many
segments for it."""
import numpy as np

from oracle import hmm_vb_oracle as orc
from test_gpu_hmmseg import random_posterior

D = 2
PIVOT = np.array([0.25, -0.5])


def seg_ahead(K):
    """kSegAhead<KT> of csrc/hmmseg_kernels.h: the rho' rows a forward wave keeps in flight."""
    return 4 if (K + 15) // 16 <= 2 else 2


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def rows(K, T, seed):
    return orc.synth_hmm(max(2, K // 2), D, T, np.float64, seed=seed, stay=0.8)[0]


def edge_lengths(K, S=20):
    """kSegAhead - 1, kSegAhead, kSegAhead + 1, twice it, twice it + 1, 0, 1, 2, cycled."""
    a = seg_ahead(K)
    return np.array([[a - 1, a, a + 1, 2 * a, 2 * a + 1, 0, 1, 2][i % 8] for i in range(S)])


def empty_sheaf_lengths(ends_empty, S=40):
    """18 sequences of 1 .. 7 rows scattered among 22 empty ones: sorted by length, sheaf 0 is full, sheaf 1 mixed (2 members
    with rows) and sheaf 2 has only empty members.  ``ends_empty``: the first and the last sequence are empty."""
    lengths = np.zeros(S, dtype=np.int64)
    at = np.array([0, 3, 4, 7, 9, 10, 13, 16, 18, 21, 22, 25, 28, 30, 33, 34, 37, 39])
    if ends_empty:
        at = np.where(at == 0, 1, np.where(at == 39, 38, at))
    lengths[at] = 1 + np.arange(18) % 7
    return lengths


def long_member_lengths(at):
    """Sixteen sequences: one of 120 rows at position ``at`` among fifteen of 1 .. 5 rows."""
    lengths = 1 + np.arange(16) % 5
    lengths[at] = 120
    return lengths


def long_member_order(column):
    """The 120-row sequence (position 7) as column ``column`` of the one sheaf, the others in their order."""
    rest = [s for s in range(16) if s != 7]
    return np.array(rest[:column] + [7] + rest[column:], dtype=np.int32)


def many_sheaves_lengths(S=65 + 64):
    """129 sequences of 0 .. 3 rows: nine sheaves, and with room for four slabs wave 0 takes sheaves 0, 4 and 8."""
    return np.array([[1, 2, 0, 3, 1, 0, 2, 1][i % 8] for i in range(S)])


def sparse_prior(q):
    """pi~ with one exact zero; row 2 of A~ with two exact zeros and one entry of 1e-40."""
    q.pi_tilde = q.pi_tilde.copy()
    q.a_tilde = q.a_tilde.copy()
    q.pi_tilde[1] = 0.0
    q.a_tilde[2, 0] = q.a_tilde[2, 3] = 0.0
    q.a_tilde[2, 1] = 1e-40
    return q


def _exact_cases():
    out = []
    for K in (1, 2, 16, 17, 32, 33, 48, 49, 64):
        out.append(dict(name=f"edges-K{K}", K=K, lengths=edge_lengths(K)))
    for K in (16, 32, 33):
        out.append(dict(name=f"empty-sheaf-K{K}", K=K, lengths=empty_sheaf_lengths(False)))
        out.append(dict(name=f"empty-sheaf-ends-K{K}", K=K, lengths=empty_sheaf_lengths(True)))
        out.append(dict(name=f"empty-sheaf-arange-K{K}", K=K, lengths=empty_sheaf_lengths(False), order=np.arange(40, dtype=np.int32)))
    for K in (3, 33):
        for column in (0, 15):
            out.append(dict(name=f"long-member-K{K}-column{column}", K=K, lengths=long_member_lengths(7),
                            order=long_member_order(column)))
    for K in (16, 17):
        out.append(dict(name=f"three-sheaves-a-wave-K{K}", K=K, lengths=many_sheaves_lengths(), switch="GMMVB_HMMSEG_WAVES"))
    out.append(dict(name="empty-sheaf-xi-separate-K17", K=17, lengths=empty_sheaf_lengths(False), switch="GMMVB_HMM_XI_SEPARATE"))
    out.append(dict(name="exact-zeros-K4", K=4, lengths=edge_lengths(4, S=17), prior=sparse_prior))
    return out


EXACT = _exact_cases()
EXACT_NAMES = [c["name"] for c in EXACT]


def inputs(case):
    """(x, q, off, order) of a case; x and q depend on K and the lengths alone."""
    K, off = case["K"], offsets(case["lengths"])
    q = random_posterior(K, D)
    if case.get("prior"):
        q = case["prior"](q)
    return rows(K, int(off[-1]), seed=K + len(off)), q, off, case.get("order")


# ---- binary64-oracle cases ------------------------------------------------------------------------------------------------------
ONES = [(K, S) for K in (3, 33) for S in (1, 16, 17, 65)]          # every sequence one row: T = S, no transition at all
REUSE = (17, 33)                                                    # 65 sequences with transitions, then 5 of one row


def room_sequences(T, K):
    """A sequence count whose ceil(S / 64) exceeds the room run_segments has for partial sums, (npad / 16 + 2) Kp / 2 with
    npad the rows padded to 64 (csrc/workspace_plan.h) - the `room` cap of n_part, below its cap of 256."""
    npad, kp = (T + 63) // 64 * 64, 16 * ((K + 15) // 16)
    room = (npad // 16 + 2) * kp // 2
    assert room < 256
    return 64 * (room + 2), room


def ends_lengths(which):
    if which == "cap":                                              # n_part = 256, per = 65: blocks 253 .. 255 start past n_seq
        return np.array([[1, 2, 0, 3][i % 4] for i in range(16400)])
    some = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 1])                 # "room": ten sequences with rows among thousands without
    S, _ = room_sequences(int(some.sum()), 3)
    lengths = np.zeros(S, dtype=np.int64)
    lengths[np.linspace(5, S - 7, 10).astype(np.int64)] = some
    return lengths


def batched_oracle(x, q, off):
    """segment_oracle of tests/test_gpu_hmmseg.py with the segments of one length walked together (the reference's scaled
    recursions, vectorised over the segments of a length class): gamma, ms, g0, gl, lnc."""
    T, K = x.shape[0], q.m.shape[0]
    ln_rho = orc.emission_ln_rho(x.astype(np.float64), q)
    mx = ln_rho.max(axis=1)
    rho = np.exp(ln_rho - mx[:, None])
    lengths, pi, a = np.diff(off), q.pi_tilde, q.a_tilde
    gamma, ms, g0, gl, lnc = np.zeros((T, K)), np.zeros((K, K)), np.zeros(K), np.zeros(K), float(mx.sum())
    for n in np.unique(lengths[lengths > 0]):
        idx = off[:-1][lengths == n][:, None] + np.arange(n)[None]          # [segments, n] rows
        r = rho[idx]
        al, be, c = np.empty_like(r), np.ones_like(r), np.empty(idx.shape)
        for t in range(n):
            v = r[:, t] * (pi[None] if t == 0 else al[:, t - 1] @ a)
            c[:, t] = v.sum(axis=1)
            al[:, t] = v / c[:, t, None]
        for t in range(n - 2, -1, -1):
            be[:, t] = (r[:, t + 1] * be[:, t + 1]) @ a.T / c[:, t + 1, None]
        g = al * be
        gamma[idx] = g
        for t in range(1, n):
            ms += (al[:, t - 1].T @ (r[:, t] * be[:, t] / c[:, t, None])) * a
        g0, gl, lnc = g0 + g[:, 0].sum(axis=0), gl + g[:, -1].sum(axis=0), lnc + float(np.log(c).sum())
    return dict(gamma=gamma, ms=ms, g0=g0, gl=gl, lnc=lnc, ns=gamma.sum(axis=0))
