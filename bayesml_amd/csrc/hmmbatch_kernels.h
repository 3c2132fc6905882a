// Predictive log-density of many independent sequences under one HMM (include/hmmbatch.h): the recursion and its closing.
// rho' [n_rows][Kp] (lane order) and m [n_rows] of the concatenated rows are hmmpred's (hmmpred_emit.h).
//
//   batch_walk_mfma_kernel<KT> : up to 64 states.  A wave owns a SHEAF of 16 sequences, consecutive in `order`, as the 16
//                                columns of v_mfma_f64_16x16x4_f64 and steps them together.  The orientation is hmm.h's,
//                                Phi^T <- A^T Phi^T: the state vectors live in the C/D layout (state 16 it + g + 4 r in
//                                register r of tile it, sequence on lane & 15), the contraction index of MFMA s of block kt
//                                is 16 kt + g + 4 s, and so the accumulator of one step IS the B operand of the next - no
//                                cross-lane move, no LDS, no barrier in the whole recursion.  A^T is held as A-operand
//                                fragments in registers (load_aop), read once per wave.  A sequence start is exact: step 0
//                                closes w0 directly, nothing is swept or gated, and phi never leaves the registers - ln p,
//                                z and the last phi of each sequence are all that is stored.
//   batch_walk_wide_kernel     : 65 .. 256 states: a workgroup per sequence, a thread per state, walk_kernel's step.
//   segment_totals_kernel      : a wave per sequence sums its ln p in a fixed order.
#pragma once
#include "hmm.h"

namespace hmmbatch {

using gmmvb::d4;
using gmmvb::hmm_pos;

constexpr int kSheaf = 16;             // sequences per wave: the MFMA's column count
constexpr int kWavesPerGroup = 4;
constexpr int kWideThreads = 256;      // HMMBATCH_MAX_STATES: a thread per state

// Steps whose rho' rows and m a wave keeps in flight in registers.  The addresses do not depend on phi, only the arithmetic
// does: with the rows of the next steps already under way a step costs its dependent MFMA chain and not a memory round trip.
// 4 KT doubles per step and lane; at three and four blocks the A fragments (4 KT^2 doubles per lane) leave room for two.
template <int KT>
constexpr int kAhead = KT <= 2 ? 4 : 2;

__device__ __forceinline__ int64_t wave_uniform(int64_t v) {      // v is the same in every lane: move it to scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v & 0xffffffffu));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// (value, state) of the larger value, the lower state on a tie: commutative and associative, so every lane of a butterfly
// ends with the same pair
__device__ __forceinline__ void take_first_max(double& v, int& k, double ov, int ok) {
    if (ov > v || (ov == v && ok < k)) {
        v = ov;
        k = ok;
    }
}

template <int KT>
__global__ __launch_bounds__(64 * kWavesPerGroup) void batch_walk_mfma_kernel(
    const double* __restrict__ rho_tm, const double* __restrict__ mx, const double* __restrict__ a, int K,
    const int64_t* __restrict__ off, const int32_t* __restrict__ order, int64_t n_seq, const double* __restrict__ w0,
    int64_t w0_stride, double* __restrict__ lnp, int64_t* __restrict__ z, double* __restrict__ end) {
    constexpr int Kp = 16 * KT;
    constexpr int PF = kAhead<KT>;
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int64_t sheaf = (int64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
    if (sheaf * kSheaf >= n_seq) return;                            // (the whole wave)
    const int64_t idx = sheaf * kSheaf + j;
    const bool live = idx < n_seq;
    const int64_t n = live ? (int64_t)order[idx] : 0;
    const int64_t lo = live ? off[n] : 0;
    const int64_t len = live ? off[n + 1] - lo : 0;
    // the sheaf steps to the end of its longest member (its first, where `order` is sorted; no order is relied upon)
    int64_t longest = len;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const int64_t other = __shfl_xor(longest, o);
        longest = other > longest ? other : longest;
    }
    const int64_t steps = wave_uniform(longest);

    double aop[KT][KT][4];
    gmmvb::load_aop<KT>(a, K, /*transpose=*/true, K, aop);          // phi^T_new = A^T phi^T_old
    d4 al[KT];                                                      // the member's vector: w0, then phi of its last step so far
    const double* w0n = w0 + n * w0_stride;
#pragma unroll
    for (int it = 0; it < KT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) al[it][r] = (live && 16 * it + g + 4 * r < K) ? w0n[16 * it + g + 4 * r] : 0.0;

    if (steps > 0) {                                                // (then there is a row 0 to clamp to)
        d4 rbuf[PF][KT];
        double mbuf[PF];
        auto fetch = [&](int64_t t, d4 (&dst)[KT], double& m) {     // (unconditional loads from a clamped row: hmm.h, H4)
            const int64_t row = t < len ? lo + t : 0;
#pragma unroll
            for (int it = 0; it < KT; ++it) dst[it] = *reinterpret_cast<const d4*>(rho_tm + row * Kp + 16 * it + 4 * g);
            m = mx[row];
        };
#pragma unroll
        for (int p = 0; p < PF; ++p) fetch(p, rbuf[p], mbuf[p]);
        for (int64_t t0 = 0; t0 < steps; t0 += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int64_t t = t0 + p;
                if (t >= steps) break;
                const bool on = t < len;                            // a member that has ended: no stores, its vector frozen
                d4 nw[KT];
                if (t == 0) {                                       // step 0 closes w0 directly
#pragma unroll
                    for (int it = 0; it < KT; ++it) nw[it] = al[it];
                } else {
                    gmmvb::apply<KT>(aop, al, nw);
                }
                d4 rho[KT];
#pragma unroll
                for (int it = 0; it < KT; ++it) rho[it] = rbuf[p][it];
                const double m = mbuf[p];
                fetch(t + PF, rbuf[p], mbuf[p]);                    // the slot's next tenant
                double part = 0.0;
#pragma unroll
                for (int it = 0; it < KT; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        nw[it][r] *= rho[it][r];
                        part += nw[it][r];
                    }
                const double s = gmmvb::sum_groups(part);           // ((g0 + g1) + (g2 + g3)) of the lanes' fixed-order sums
                double best = -1.0;
                int arg = 0;
#pragma unroll
                for (int it = 0; it < KT; ++it)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double phi = s > 0.0 ? nw[it][r] / s : 0.0;
                        if (phi > best) {                           // (a lane's states ascend with it, r: the first maximum)
                            best = phi;
                            arg = 16 * it + g + 4 * r;
                        }
                        al[it][r] = on ? phi : al[it][r];
                    }
                if (z != nullptr) {                                 // (padded states hold 0 and lie above every state: never first)
                    take_first_max(best, arg, __shfl_xor(best, 16), __shfl_xor(arg, 16));
                    take_first_max(best, arg, __shfl_xor(best, 32), __shfl_xor(arg, 32));
                }
                if (on && g == 0) {
                    lnp[lo + t] = log(s) + m;
                    if (z != nullptr) z[lo + t] = arg;
                }
            }
        }
    }
    if (live) {                                                     // an empty sequence: its start vector
#pragma unroll
        for (int it = 0; it < KT; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * it + g + 4 * r < K) end[n * K + 16 * it + g + 4 * r] = al[it][r];
    }
}

// 65 .. 256 states: walk_kernel's step between off[n] and off[n + 1], a workgroup per sequence (blockIdx.x-th of `order`).
__global__ __launch_bounds__(kWideThreads) void batch_walk_wide_kernel(
    const double* __restrict__ rho_tm, const double* __restrict__ mx, const double* __restrict__ a, int K, int Kp,
    const int64_t* __restrict__ off, const int32_t* __restrict__ order, const double* __restrict__ w0, int64_t w0_stride,
    double* __restrict__ lnp, int64_t* __restrict__ z, double* __restrict__ end) {
    __shared__ double cur[kWideThreads];
    __shared__ double red[4];
    __shared__ double bestv[4];
    __shared__ int bestk[4];
    const int tid = threadIdx.x;
    const bool state = tid < K;
    const int pos = hmm_pos(tid < Kp ? tid : 0);
    const int64_t n = order[blockIdx.x];
    const int64_t lo = off[n], len = off[n + 1] - lo;
    cur[tid] = state ? w0[n * w0_stride + tid] : 0.0;
    __syncthreads();
    for (int64_t t = 0; t < len; ++t) {
        double w = cur[tid];                                        // step 0: w0 itself
        if (t > 0 && state) {
            w = 0.0;
            for (int jj = 0; jj < K; ++jj) w = fma(cur[jj], a[(int64_t)jj * K + tid], w);
        }
        const double v = state ? w * rho_tm[(lo + t) * Kp + pos] : 0.0;
        double s = gmmvb::sum_wave(v);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();                                            // (every thread has read cur)
        s = (red[0] + red[1]) + (red[2] + red[3]);
        const double phi = s > 0.0 ? v / s : 0.0;
        cur[tid] = phi;
        if (z != nullptr) {
            double best = state ? phi : -1.0;
            int arg = tid;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) take_first_max(best, arg, __shfl_xor(best, o), __shfl_xor(arg, o));
            if ((tid & 63) == 0) {
                bestv[tid >> 6] = best;
                bestk[tid >> 6] = arg;
            }
        }
        __syncthreads();                                            // (cur is whole; red is free again)
        if (tid == 0) {
            lnp[lo + t] = log(s) + mx[lo + t];
            if (z != nullptr) {
                double best = bestv[0];
                int arg = bestk[0];
                for (int wv = 1; wv < 4; ++wv) take_first_max(best, arg, bestv[wv], bestk[wv]);
                z[lo + t] = arg;                                    // (read before the next step's first barrier rewrites them)
            }
        }
    }
    if (state) end[n * K + tid] = cur[tid];
}

// tot[n] = sum of lnp[off[n] .. off[n + 1]): lane l adds the entries l, l + 64, .. in order, then the butterfly.
__global__ __launch_bounds__(64 * kWavesPerGroup) void segment_totals_kernel(const int64_t* __restrict__ off,
                                                                             const double* __restrict__ lnp, int64_t n_seq,
                                                                             double* __restrict__ tot) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
    if (n >= n_seq) return;
    const int64_t lo = off[n], hi = off[n + 1];
    double acc = 0.0;
    for (int64_t t = lo + lane; t < hi; t += 64) acc += lnp[t];
    acc = gmmvb::sum_wave(acc);
    if (lane == 0) tot[n] = acc;
}

}  // namespace hmmbatch
