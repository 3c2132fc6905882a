// Viterbi over many independent sequences laid end to end (hmmvb_viterbi_segments, up to 64 states).
// lnrho [K][npad] is the emission array of the last E-step, off [n_seq + 1] the row offsets of the sequences and
// order [n_seq] the order in which the waves take them (hmmseg_kernels.h's tables).
//
//   hmmvit_segments_kernel<Kq> : Kq = the smallest of 4, 8, 16, 32, 64 that holds the K states.  A wave owns a PACK of
//                                G = 64 / Kq sequences, consecutive in `order`: lane = (member m = lane / Kq, state
//                                j = lane % Kq), so at K <= 32 the lanes the single-chain kernel leaves idle carry other
//                                chains.  Lane (m, j) holds column j of ln a~ (Kq doubles) and keeps 8 steps of its own
//                                state's ln rho ahead.  Per step every lane needs the Kq omega values of its member:
//                                at G = 1 by readlane (a uniform-index shuffle), at G > 1 through a wave-private LDS line of
//                                64 doubles (one 8-byte write per lane, Kq / 2 16-byte reads that are broadcasts within a
//                                member), two lines in turn so that one wave-level ordering point per step is enough.
//                                The recursion is the reference's in the reference's order - v_i = omega_i + ln a~_ij,
//                                the first maximiser over i ascending, omega_j = ln rho_tj + best - so a path is the
//                                sequential one bit for bit whatever the pack, the order or the neighbours.
//                                The same wave then backtracks its members: the final state is the first maximiser of the
//                                member's last omega (a reduction over its own Kq lanes, the lower index on ties), the
//                                back-pointer rows are staged into wave-private LDS in blocks of 64 steps from the end
//                                backwards, and one lane per member chases them, all G members at once.
// A member that has ended (or is empty) is masked: no stores, omega frozen by a select.  Padded entries of ln a~ and the
// omega of padded states carry hmm.h's sentinel -1e300 and never win a maximum.
#pragma once
#include "hmm.h"

namespace gmmvb {

constexpr int kVitSegWaves = 4;            // waves per workgroup
constexpr int kVitSegAhead = 8;            // steps of ln rho a lane keeps in flight (hmm_viterbi_forward_kernel's 8)
constexpr int kVitSegBlock = 64;           // steps of back-pointers per staged block

// wave-level ordering of the wave's own LDS lines (no other wave reads them)
__device__ __forceinline__ void vit_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane i's value in scalar registers (i is a compile-time constant after unrolling: two readlanes, where __shfl left the
// compiler free to go through the LDS crossbar)
__device__ __forceinline__ double vit_lane_value(double v, int i) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)(b & 0xffffffffu), i);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), i);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// the largest of the 64 lanes' values, in every lane (scalar)
__device__ __forceinline__ int64_t vit_wave_max(int64_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t other = __shfl_xor(v, o);
        v = other > v ? other : v;
    }
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v & 0xffffffffu));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <int Kq>
__global__ __launch_bounds__(64 * kVitSegWaves) void hmmvit_segments_kernel(
    const double* __restrict__ lnrho, int64_t npad, const double* __restrict__ ln_pi_tilde,
    const double* __restrict__ ln_a_tilde, int K, int Kp, const int64_t* __restrict__ off,
    const int32_t* __restrict__ order, int64_t n_seq, unsigned char* __restrict__ phi /*[npad][Kp]*/,
    int32_t* __restrict__ z) {
    constexpr int G = 64 / Kq;
    constexpr double NEG = -1.0e300;
    // the omega lines (G > 1) and the staged back-pointer blocks, both private to a wave
    __shared__ __attribute__((aligned(16))) double lines[G > 1 ? kVitSegWaves * 2 * 64 : 2];
    __shared__ __attribute__((aligned(16))) unsigned char stage[kVitSegWaves * 64 * kVitSegBlock];      // G * Kq = 64 bytes a step
    const int lane = threadIdx.x & 63, m = lane / Kq, j = lane % Kq;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t pack = (int64_t)blockIdx.x * kVitSegWaves + wv;
    if (pack * G >= n_seq) return;                                  // (the whole wave)
    const int64_t idx = pack * G + m;
    const bool live = idx < n_seq;
    const int64_t n = live ? (int64_t)order[idx] : 0;
    const int64_t lo = live ? off[n] : 0;
    const int64_t len = live ? off[n + 1] - lo : 0;
    const int64_t steps = vit_wave_max(len);
    if (steps == 0) return;                                         // (only empty members: no row to clamp to either)

    // ---- forward ------------------------------------------------------------------------------------------------------
    const bool real = j < K;
    double col[Kq];
#pragma unroll
    for (int i = 0; i < Kq; ++i) col[i] = (i < K && real) ? ln_a_tilde[i * K + j] : NEG;
    const double* lr = lnrho + (int64_t)(real ? j : 0) * npad;
    auto fetch = [&](int64_t t) { return lr[t < len ? lo + t : 0]; };      // (unconditional loads from a clamped row)
    double omega = (real && len > 0) ? fetch(0) + ln_pi_tilde[j] : NEG;
    double e[kVitSegAhead];
#pragma unroll
    for (int u = 0; u < kVitSegAhead; ++u) e[u] = fetch(1 + u);
    double* const line = lines + (G > 1 ? wv * 2 * 64 : 0);
    for (int64_t t0 = 1; t0 < steps; t0 += kVitSegAhead) {
#pragma unroll
        for (int u = 0; u < kVitSegAhead; ++u) {
            const int64_t t = t0 + u;
            if (t >= steps) break;
            const bool on = t < len;                                // a member that has ended: no stores, omega frozen
            const double em = e[u];
            e[u] = fetch(t + kVitSegAhead);                         // the slot's next tenant
            double best = NEG * 2.0;
            int arg = 0;
            if constexpr (G == 1) {
#pragma unroll
                for (int i = 0; i < Kq; ++i) {
                    const double v = vit_lane_value(omega, i) + col[i];
                    if (v > best) {          // strict: first maximiser, like numpy.argmax
                        best = v;
                        arg = i;
                    }
                }
            } else {
                double* const ln = line + (u & 1) * 64;             // (kVitSegAhead is even: the lines alternate across t0 too)
                ln[lane] = omega;
                vit_wave_sync();
                const double2* mine = reinterpret_cast<const double2*>(ln + m * Kq);
#pragma unroll
                for (int i = 0; i < Kq; i += 2) {
                    const double2 w = mine[i / 2];
                    const double v0 = w.x + col[i], v1 = w.y + col[i + 1];
                    if (v0 > best) {
                        best = v0;
                        arg = i;
                    }
                    if (v1 > best) {
                        best = v1;
                        arg = i + 1;
                    }
                }
            }
            const double nw = real ? em + best : NEG;
            omega = on ? nw : omega;
            if (on && real) phi[(lo + t) * Kp + j] = (unsigned char)arg;
        }
    }

    // ---- the members' final states: first maximiser of the last omega over the member's own Kq lanes ----------------------
    double best = omega;
    int cur = j;
#pragma unroll
    for (int o = Kq / 2; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(cur, o);
        if (ob > best || (ob == best && oa < cur)) {
            best = ob;
            cur = oa;
        }
    }

    // ---- backtrack: the wave reads back-pointers its own lanes stored --------------------------------------------------
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const bool chaser = j == 0 && len > 0;
    if (chaser) z[lo + len - 1] = cur;
    const int words = (Kq < Kp ? Kq : Kp) / 4;                      // 4-byte words of a step that phi holds (K = 33 .. 48: Kp = 48 < Kq)
    unsigned char* const st = stage + (wv * 64 + m * Kq) * kVitSegBlock;      // [kVitSegBlock][Kq] of this member
    // block b of a member: steps hi = len - 1 - 64 b down to max(1, hi - 63); phi[t] gives the state at t - 1
    for (int64_t b0 = 0; b0 < steps - 1; b0 += kVitSegBlock) {
        const int64_t hi = len - 1 - b0;
        const int64_t lw = hi - (kVitSegBlock - 1) > 1 ? hi - (kVitSegBlock - 1) : 1;
        const int rows = hi >= 1 ? (int)(hi - lw + 1) : 0;           // (0: this member has no step left)
        for (int el = j; el < rows * words; el += Kq) {
            const int s = el / words, w = el % words;
            *reinterpret_cast<unsigned*>(st + s * Kq + 4 * w) =
                *reinterpret_cast<const unsigned*>(phi + (lo + lw + s) * Kp + 4 * w);
        }
        vit_wave_sync();
        if (chaser) {
            for (int s = rows - 1; s >= 0; --s) {
                cur = st[s * Kq + cur];
                z[lo + lw + s - 1] = cur;
            }
        }
        vit_wave_sync();
    }
}

}  // namespace gmmvb
