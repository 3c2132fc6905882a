// Forward-backward over many independent sequences laid end to end (hmmvb_forward_backward_segments, up to 64 states).
// The rows, rho' [npad][Kp] (lane order), mx, alpha_tm, gamma_tm, w_tm, cprime are hmm.h's; off [n_seq + 1] are the row
// offsets of the sequences and order [n_seq] the order in which the waves take them.
//
//   hmmseg_forward_kernel<KT>      : a wave owns a SHEAF of 16 sequences, consecutive in `order`, as the 16 columns of
//                                    v_mfma_f64_16x16x4_f64 (hmmbatch_kernels.h's membership, hmm.h's orientation
//                                    alpha^T <- A~^T alpha^T: the accumulator of one step is the B operand of the next).
//                                    Every sequence start is an exact boundary: step 0 closes rho'_0 o pi~ directly, so
//                                    nothing is swept, gated or repaired.  Writes alpha and c' of every row.
//   hmmseg_backward_kernel<KT, XI> : the same membership; every member walks back from its OWN last row (beta = 1 there), so
//                                    at wave step i member j is at row end_j - 1 - i.  Writes gamma; the xi sum either inside
//                                    (XI, up to 32 states: the 16 members as the contraction index, hmm.h H5) into one slab
//                                    per wave, or as w_tm with w = 0 at every first row for hmm_xi_sum_kernel.
//   hmmseg_ends_*_kernel           : g0 / gl, the sums of gamma over the sequences' first / last rows, in a fixed order.
// A member that has ended is masked: no stores, its registers frozen by a select.  No column of an MFMA depends on another,
// and sum_groups adds the four lane groups of one column: alpha, c', gamma and w of a row are the same bits whatever the
// order, the sheaf or the neighbours.  The xi slabs and the g0 / gl partial sums add members in the order given: equal to
// rounding.
#pragma once
#include "hmm.h"

namespace gmmvb {

constexpr int kSegSheaf = 16;          // sequences per wave: the MFMA's column count
constexpr int kSegWaves = 4;           // waves per workgroup
constexpr int kSegEndsSeqs = 64;       // sequences per workgroup of hmmseg_ends_partial_kernel, at least

// steps whose rho' rows a forward wave keeps in flight (hmmbatch_kernels.h, kAhead: the A fragments of three and four
// blocks leave room for two)
template <int KT>
constexpr int kSegAhead = KT <= 2 ? 4 : 2;

__device__ __forceinline__ int64_t seg_wave_uniform(int64_t v) {      // v is the same in every lane: to scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v & 0xffffffffu));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the largest of the 16 members' lengths, in every lane
__device__ __forceinline__ int64_t seg_longest(int64_t len) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const int64_t other = __shfl_xor(len, o);
        len = other > len ? other : len;
    }
    return seg_wave_uniform(len);
}

template <int KT>
__global__ __launch_bounds__(64 * kSegWaves) void hmmseg_forward_kernel(
    const double* __restrict__ rho_tm, const double* __restrict__ pi_tilde, const double* __restrict__ a_tilde, int K,
    const int64_t* __restrict__ off, const int32_t* __restrict__ order, int64_t n_seq, double* __restrict__ alpha_tm,
    double* __restrict__ cprime) {
    constexpr int Kp = 16 * KT;
    constexpr int PF = kSegAhead<KT>;
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int64_t sheaf = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
    if (sheaf * kSegSheaf >= n_seq) return;                         // (the whole wave)
    const int64_t idx = sheaf * kSegSheaf + j;
    const bool live = idx < n_seq;
    const int64_t n = live ? (int64_t)order[idx] : 0;
    const int64_t lo = live ? off[n] : 0;
    const int64_t len = live ? off[n + 1] - lo : 0;
    const int64_t steps = seg_longest(len);
    if (steps == 0) return;                                         // (only empty members: no row to clamp to either)

    double aop[KT][KT][4];
    load_aop<KT>(a_tilde, K, /*transpose=*/true, K, aop);           // alpha^T_new = A~^T alpha^T_old
    d4 al[KT];                                                      // pi~, then the member's alpha of its last step so far
#pragma unroll
    for (int it = 0; it < KT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) al[it][r] = (live && 16 * it + g + 4 * r < K) ? pi_tilde[16 * it + g + 4 * r] : 0.0;

    d4 rbuf[PF][KT];
    auto fetch = [&](int64_t t, d4 (&dst)[KT]) {                    // (unconditional loads from a clamped row: hmm.h, H4)
        const int64_t row = t < len ? lo + t : 0;
#pragma unroll
        for (int it = 0; it < KT; ++it) dst[it] = *reinterpret_cast<const d4*>(rho_tm + row * Kp + 16 * it + 4 * g);
    };
#pragma unroll
    for (int p = 0; p < PF; ++p) fetch(p, rbuf[p]);
    for (int64_t t0 = 0; t0 < steps; t0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int64_t t = t0 + p;
            if (t >= steps) break;
            const bool on = t < len;                                // a member that has ended: no stores, alpha frozen
            d4 nw[KT];
            if (t == 0) {                                           // step 0 closes pi~ directly
#pragma unroll
                for (int it = 0; it < KT; ++it) nw[it] = al[it];
            } else {
                apply<KT>(aop, al, nw);
            }
            d4 rho[KT];
#pragma unroll
            for (int it = 0; it < KT; ++it) rho[it] = rbuf[p][it];
            fetch(t + PF, rbuf[p]);                                 // the slot's next tenant
            double part = 0.0;
#pragma unroll
            for (int it = 0; it < KT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    nw[it][r] *= rho[it][r];
                    part += nw[it][r];
                }
            const double cp = sum_groups(part);
            const double inv = cp > 0.0 ? 1.0 / cp : 0.0;
#pragma unroll
            for (int it = 0; it < KT; ++it) {
#pragma unroll
                for (int r = 0; r < 4; ++r) al[it][r] = on ? nw[it][r] * inv : al[it][r];
                if (on) *reinterpret_cast<d4*>(alpha_tm + (lo + t) * Kp + 16 * it + 4 * g) = al[it];
            }
            if (on && g == 0) cprime[lo + t] = cp;
        }
    }
}

// XI: a wave takes the sheaves wave, wave + n_waves, .. (n_waves = gridDim.x * kSegWaves <= the slabs there is room for) and
// adds all their terms into its one slab; !XI: n_waves covers the sheaves, one each.
// (XI at two blocks: two waves per SIMD - at three, the step-ahead rows beside the xi accumulators spilled 96 registers)
template <int KT, bool XI>
__global__ __launch_bounds__(64 * kSegWaves, XI ? (KT == 1 ? 3 : 2) : 1) void hmmseg_backward_kernel(
    const double* __restrict__ rho_tm, const double* __restrict__ a_tilde, int K, const int64_t* __restrict__ off,
    const int32_t* __restrict__ order, int64_t n_seq, const double* __restrict__ alpha_tm, const double* __restrict__ cprime,
    double* __restrict__ gamma_tm, double* __restrict__ w_tm, double* __restrict__ xi_slabs) {
    constexpr int Kp = 16 * KT;
    constexpr int LDW = hmm_xi_ldw(Kp);
    __shared__ __attribute__((aligned(16))) double xs[XI ? kSegWaves * 2 * 16 * LDW : 2];
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    double* const sa = xs + (XI ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 2 * 16 * LDW : 0);
    double* const sb = sa + (XI ? 16 * LDW : 0);
    d4 xacc[XI ? KT : 1][XI ? KT : 1];
    if constexpr (XI) {
#pragma unroll
        for (int it = 0; it < KT; ++it)
#pragma unroll
            for (int jt = 0; jt < KT; ++jt) xacc[it][jt] = d4{0.0, 0.0, 0.0, 0.0};
    }
    // xacc += sum over the wave's members of al (x) wv   (hmm.h, H5: both operands transposed through the wave's LDS tile)
    auto xi_add = [&](const d4 (&al)[KT], const d4 (&wv)[XI ? KT : 1]) {
        if constexpr (XI) {
#pragma unroll
            for (int it = 0; it < KT; ++it) {
                *reinterpret_cast<d4*>(sa + j * LDW + 16 * it + 4 * g) = al[it];
                *reinterpret_cast<d4*>(sb + j * LDW + 16 * it + 4 * g) = wv[it];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double a[KT], b[KT];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    a[kt] = sa[(4 * q + g) * LDW + 16 * kt + j];
                    b[kt] = sb[(4 * q + g) * LDW + 16 * kt + j];
                }
#pragma unroll
                for (int it = 0; it < KT; ++it)
#pragma unroll
                    for (int jt = 0; jt < KT; ++jt) xacc[it][jt] = mfma_f64(a[it], b[jt], xacc[it][jt]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };
    const int64_t wave = (int64_t)blockIdx.x * kSegWaves + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kSegWaves;
    const int64_t n_sheaves = (n_seq + kSegSheaf - 1) / kSegSheaf;
    double aop[KT][KT][4];
    load_aop<KT>(a_tilde, K, /*transpose=*/false, K, aop);          // beta_{t-1} ~ A~ (rho'_t o beta_t)

    for (int64_t sheaf = wave; sheaf < n_sheaves; sheaf += n_waves) {
        const int64_t idx = sheaf * kSegSheaf + j;
        const bool live = idx < n_seq;
        const int64_t n = live ? (int64_t)order[idx] : 0;
        const int64_t lo = live ? off[n] : 0;
        const int64_t len = live ? off[n + 1] - lo : 0;
        const int64_t steps = seg_longest(len);
        d4 be[KT];                                                  // beta = 1 behind every member's last row
#pragma unroll
        for (int it = 0; it < KT; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) be[it][r] = 16 * it + g + 4 * r < K ? 1.0 : 0.0;
        d4 wprev[XI ? KT : 1];
        // the rows of step i: alpha, rho' and c' of row lo + len - 1 - i, zero / one where the member has ended; requested a
        // step ahead (the addresses do not depend on beta)
        d4 al_n[KT], rho_n[KT];
        double cp_n;
        auto fetch = [&](int64_t i) {
            const bool on = i < len;
            const int64_t row = on ? lo + len - 1 - i : 0;
#pragma unroll
            for (int it = 0; it < KT; ++it) {
                al_n[it] = d4{0.0, 0.0, 0.0, 0.0};
                rho_n[it] = d4{0.0, 0.0, 0.0, 0.0};
                if (on) {
                    al_n[it] = *reinterpret_cast<const d4*>(alpha_tm + row * Kp + 16 * it + 4 * g);
                    rho_n[it] = *reinterpret_cast<const d4*>(rho_tm + row * Kp + 16 * it + 4 * g);
                }
            }
            cp_n = on ? cprime[row] : 1.0;
        };
        if (steps > 0) fetch(0);
        for (int64_t i = 0; i < steps; ++i) {
            const bool on = i < len;
            const bool first = i + 1 == len;                        // the member is at its first row: xi = 0 there
            const int64_t row = lo + len - 1 - i;
            d4 al[KT], rho[KT];
#pragma unroll
            for (int it = 0; it < KT; ++it) {
                al[it] = al_n[it];
                rho[it] = rho_n[it];
            }
            const double cp = cp_n;
            fetch(i + 1);
            // gamma_t, w_t from beta_t (registers), alpha_t, rho'_t, c'_t
            double dot = 0.0;
#pragma unroll
            for (int it = 0; it < KT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) dot = fma(al[it][r], be[it][r], dot);
            dot = sum_groups(dot);
            const double ginv = dot > 0.0 ? 1.0 / dot : 0.0;
            const double winv = (on && !first && dot > 0.0 && cp > 0.0) ? 1.0 / (dot * cp) : 0.0;
            d4 y[KT], wnow[XI ? KT : 1];
#pragma unroll
            for (int it = 0; it < KT; ++it) {
                d4 gm, ww;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    y[it][r] = rho[it][r] * be[it][r];
                    gm[r] = al[it][r] * be[it][r] * ginv;
                    ww[r] = y[it][r] * winv;                        // (zero at a first row and where the member has ended)
                }
                if (on) {
                    *reinterpret_cast<d4*>(gamma_tm + row * Kp + 16 * it + 4 * g) = gm;
                    if constexpr (!XI) *reinterpret_cast<d4*>(w_tm + row * Kp + 16 * it + 4 * g) = ww;
                }
                if constexpr (XI) wnow[it] = ww;
            }
            if constexpr (XI) {
                if (i > 0) xi_add(al, wprev);                       // the term of the row behind: alpha_t (x) w_{t+1}
#pragma unroll
                for (int it = 0; it < KT; ++it) wprev[it] = wnow[it];
            }
            // beta_{t-1} ~ A~ y, renormalised to sum 1 (a member that has ended keeps its vector)
            d4 nb[KT];
            apply<KT>(aop, y, nb);
            double part = 0.0;
#pragma unroll
            for (int it = 0; it < KT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) part += nb[it][r];
            const double tot = sum_groups(part);
            const double inv = tot > 0.0 ? 1.0 / tot : 0.0;
#pragma unroll
            for (int it = 0; it < KT; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) be[it][r] = on ? nb[it][r] * inv : be[it][r];
        }
        // (no term is left over: at the wave's last step every member is at its first row or has ended, w = 0 for both)
    }
    if constexpr (XI) {
        double* out = xi_slabs + wave * Kp * Kp;
#pragma unroll
        for (int it = 0; it < KT; ++it)
#pragma unroll
            for (int jt = 0; jt < KT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(16 * it + g + 4 * r) * Kp + 16 * jt + j] = xacc[it][jt][r];
    }
}

// partial[b] = [sum of gamma at the first rows | at the last rows] ([2][K], natural state order) of the non-empty sequences
// b * per .. (b + 1) * per - 1: wave w adds the sequences w, w + 4, .. of the slice in order (lane = state), the four waves'
// sums are added in wave order.
__global__ __launch_bounds__(256) void hmmseg_ends_partial_kernel(const double* __restrict__ gamma_tm, int K, int Kp,
                                                                  const int64_t* __restrict__ off, int64_t n_seq, int64_t per,
                                                                  double* __restrict__ partial) {
    __shared__ double red[4][2][64];
    const int k = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pos = hmm_pos(k < K ? k : 0);
    const int64_t s_lo = (int64_t)blockIdx.x * per;
    const int64_t s_hi = s_lo + per < n_seq ? s_lo + per : n_seq;
    double first = 0.0, last = 0.0;
    for (int64_t s = s_lo + w; s < s_hi; s += 4) {
        const int64_t lo = off[s], hi = off[s + 1];
        if (hi > lo && k < K) {
            first += gamma_tm[lo * Kp + pos];
            last += gamma_tm[(hi - 1) * Kp + pos];
        }
    }
    red[w][0][k] = first;
    red[w][1][k] = last;
    __syncthreads();
    if (threadIdx.x < 128) {
        const int e = threadIdx.x >> 6;
        if (k < K) partial[((int64_t)blockIdx.x * 2 + e) * K + k] = (red[0][e][k] + red[1][e][k]) + (red[2][e][k] + red[3][e][k]);
    }
}

// out[K K ..] = [g0 | gl]: the partial sums added in block order, over the two slots hmm_finish_kernel filled from rows 0
// and T - 1
__global__ __launch_bounds__(128) void hmmseg_ends_kernel(const double* __restrict__ partial, int64_t n_partial, int K,
                                                          double* __restrict__ out) {
    const int k = threadIdx.x & 63, e = threadIdx.x >> 6;
    if (k >= K) return;
    double s = 0.0;
    for (int64_t b = 0; b < n_partial; ++b) s += partial[(b * 2 + e) * K + k];
    out[(int64_t)K * K + e * K + k] = s;
}

}  // namespace gmmvb
