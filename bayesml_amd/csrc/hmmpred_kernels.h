// Predictive log-density of a sequence under an HMM with Student-t emissions (include/hmmpred.h):
//
//   ln e_tk = c_k - a_k log1p(q_tk / nu_k),   rho'_t = exp(ln e_t - max_k ln e_tk),   w_t = phi_{t-1} A,
//   s_t = w_t . rho'_t,   ln p_t = ln s_t + m_t,   phi_t = w_t o rho'_t / s_t.
//
// What is joined here already exists: the quadratic forms are stmix_kernels.h's (quad_component over stmix_pack's image,
// staged into LDS as fused_kernel does), the recursion is hmm.h's scaled forward pass (hmm_forward_replay_body in sweep and in
// replay mode, alpha = phi and c' = s), its test hmm_boundary_check_kernel<true>.  This file adds
//   emission_kernel / emission_plain_kernel : ln e component-major [K][npad] (hmm_prep_kernel makes rho' and m of it),
//   first_step_kernel                       : step 0 closes w0 directly; shuts the gate, clears the diagnostic,
//   sweep_kernel                            : the forward sweep alone (hmm_sweeps_kernel launches both directions),
//   walk_kernel                             : ONE workgroup, a thread per state, walking steps in order - the repair behind
//                                             the gate, and the whole filter for short sequences and for 65 .. 256 states,
//   close_kernel                            : ln p, z (first maximum in natural state order) and phi_{T-1}.
#pragma once
#include "hmm.h"
#include "hmm_generic.h"
#include "stmix_kernels.h"

namespace hmmpred {

using gmmvb::d4;
using gmmvb::estep_kb;
using gmmvb::estep_nb_w;
using gmmvb::hmm_pos;
using gmmvb::img_doubles;
using stmix::kWaves;

// ---- emission, D <= 128 -----------------------------------------------------------------------------------------------------
// stmix::fused_kernel with the closing replaced: the Student-t log-kernel of every (row, state) pair is stored, component-
// major, instead of entering a running log-sum-exp (the recursion needs all K values of a row).  Same tile, same staging,
// same quad_component: q_tk has stmix_logpdf's bits.
template <int T, typename XT, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void emission_kernel(const XT* __restrict__ x, int64_t ldx, int64_t n_rows, int D,
                                                               const double* __restrict__ pivot,
                                                               const double* __restrict__ img /*[K][IMG]*/,
                                                               const double* __restrict__ cvec, const double* __restrict__ nuvec,
                                                               int K, double* __restrict__ lne /*[K][npad]*/, int64_t npad) {
    constexpr int NW = kWaves;
    constexpr int NB = estep_nb_w<double>(T, NW);
    constexpr int IMG = img_doubles(T);
    constexpr int KB = estep_kb(T);
    __shared__ __attribute__((aligned(16))) double smem[2][KB * IMG];   // the ONLY LDS object of the kernel
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int64_t rows_per_wg = NW * 16 * NB;
    const int64_t n_wg_tiles = (n_rows + rows_per_wg - 1) / rows_per_wg;
    const int n_blocks = (K + KB - 1) / KB;
    const double dims = (double)D;

    auto stage = [&](int kb, int buf) {
        const int k0 = kb * KB;
        const int kcount = (K - k0 < KB) ? (K - k0) : KB;
        const int pieces = kcount * (IMG / 128);
        const double* src = img + (int64_t)k0 * IMG + lane * 2;
        for (int piece = wave; piece < pieces; piece += NW)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 128),
                                             (__attribute__((address_space(3))) void*)(&smem[buf][piece * 128]), 16, 0,
                                             0);
    };

    for (int64_t wt = blockIdx.x; wt < n_wg_tiles; wt += gridDim.x) {
        const int64_t n0 = wt * rows_per_wg + (int64_t)wave * 16 * NB;   // may lie past n_rows: rows clamp, stores mask
        int64_t ld[NB], stv[NB];
        gmmvb::tile_rows<NB>(n0, n, n_rows, ld, stv);
        double xc[NB][T][4];
        {
            XT xr[NB][T][4];
            gmmvb::load_x_tile<T, NB, XT, VEC>(x, ldx, D, ld, g, xr);
#pragma unroll
            for (int b = 0; b < T; ++b) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int f = 16 * b + 4 * g + s;
                    const double pv = f < D ? pivot[f] : 0.0;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) xc[nb][b][s] = (double)xr[nb][b][s] - pv;
                }
            }
        }
        stage(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kb = 0; kb < n_blocks; ++kb) {
            if (kb + 1 < n_blocks) stage(kb + 1, (kb + 1) & 1);
            const double* buf = smem[kb & 1];
            const int k0 = kb * KB;
#pragma unroll 1
            for (int kk = 0; kk < KB; ++kk) {
                const int k = k0 + kk;
                if (k >= K) break;
                double q[NB];
                stmix::quad_component<NB, T>(buf + kk * IMG, xc, lane, g, q);
                const double c = cvec[k], nu = nuvec[k];
                const double a = 0.5 * (nu + dims);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const double t = c - a * log1p(q[nb] / nu);
                    if (g == 0 && stv[nb] >= 0) lne[(int64_t)k * npad + stv[nb]] = t;
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
}

// ---- emission, D > 128 ------------------------------------------------------------------------------------------------------
// stmix::plain_kernel with the same change.  Correctness only.
template <typename XT>
__global__ __launch_bounds__(64) void emission_plain_kernel(const XT* __restrict__ x, int64_t ldx, int64_t n_rows, int D,
                                                            const double* __restrict__ pivot, const double* __restrict__ img,
                                                            const double* __restrict__ cvec, const double* __restrict__ nuvec,
                                                            int K, int R, double* __restrict__ lne, int64_t npad) {
    extern __shared__ double dsh[];                           // [D][R]
    const int lane = threadIdx.x;
    const int col = lane < R ? lane : 0;
    const int64_t n_tiles = (n_rows + R - 1) / R;
    const double dims = (double)D;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * R + lane;
        const bool live = lane < R && row < n_rows;
        __syncthreads();
        if (lane < R) {
            const XT* xr = x + (live ? row : n_rows - 1) * ldx;
            for (int i = 0; i < D; ++i) dsh[(int64_t)i * R + lane] = (double)xr[i] - pivot[i];
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const double* uk = img + (int64_t)k * ((int64_t)D * D + D);
            const double* bk = uk + (int64_t)D * D;
            double q = 0.0;
            for (int j = 0; j < D; ++j) {
                const double* uj = uk + (int64_t)j * D;
                double y = bk[j];
                for (int i = 0; i <= j; ++i) y = fma(uj[i], dsh[(int64_t)i * R + col], y);
                q = fma(y, y, q);
            }
            const double nu = nuvec[k];
            if (live) lne[(int64_t)k * npad + row] = cvec[k] - 0.5 * (nu + dims) * log1p(q / nu);
        }
    }
}

// ---- the recursion ----------------------------------------------------------------------------------------------------------
constexpr int kWalkThreads = 256;      // HMMPRED_MAX_STATES: a thread per state

// sum over the workgroup in a fixed order (every thread gets it); red: [4] doubles of LDS, free again after the caller's
// next barrier
__device__ __forceinline__ double block_sum_256(double v, double* red) {
    v = gmmvb::sum_wave(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Step 0: phi_0 = w0 o rho'_0 / s_0 into row 0 of phi (lane order) and of the start vectors (natural order).  The gate is
// shut and the diagnostic cleared here, in front of everything that may set them.
__global__ __launch_bounds__(kWalkThreads) void first_step_kernel(const double* __restrict__ rho_tm, const double* __restrict__ w0,
                                                                  int K, int Kp, double* __restrict__ phi_tm,
                                                                  double* __restrict__ s_arr, double* __restrict__ starts,
                                                                  int* __restrict__ gate, int64_t* __restrict__ diag) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const double v = tid < K ? w0[tid] * rho_tm[hmm_pos(tid)] : 0.0;
    const double s = block_sum_256(v, red);
    const double phi = s > 0.0 ? v / s : 0.0;
    if (tid < Kp) {
        phi_tm[hmm_pos(tid)] = phi;
        starts[tid] = phi;
    }
    if (tid == 0) {
        s_arr[0] = s;
        *gate = 0;
        diag[0] = 0;
        diag[1] = 0;
    }
}

// The start vector of every chunk but the first from the uniform vector W steps in front of its boundary: row c + 1 of
// `starts` from the last W steps of chunk c.  (W = L: chunk 0 starts from phi_0 itself.)
template <int KT>
__global__ __launch_bounds__(256) void sweep_kernel(const double* __restrict__ rho_tm, const double* __restrict__ a, int K, int64_t T,
                                                    int64_t L, int64_t n_chunks, double* __restrict__ starts, int64_t W) {
    gmmvb::hmm_forward_replay_body<KT>(rho_tm, a, K, T, L, n_chunks, starts, nullptr, nullptr, 1, starts, L - W);
}

// hmm_boundary_check_kernel<true>'s test on one pair of entries
__device__ __forceinline__ bool entries_differ(double a, double b, double tol) {
    const double d = fabs(a - b), m = fmax(fabs(a), fabs(b));
    return !(d <= tol * m || m < 1e-290);            // (NaN: differs)
}

// The serial walk.  Chunk c = steps 1 + c L .. (c + 1) L below T; `cur` carries the filter's vector from chunk to chunk.
//   force != 0 : every chunk of [0, n_chunks) is walked from row 0 of `starts` (phi_0): the whole filter.
//   force == 0 : the repair, behind the gate.  In chunk order: a chunk whose start vector (row c of `starts`) stands against
//                the carried vector by the relative per-entry test keeps what the replay wrote, and the carried vector
//                becomes the end the replay recorded for it (row c + 1 of `ends`); any other chunk is walked again from the
//                carried vector and its phi and s rewritten.  So phi depends on forgetting only through start vectors
//                PROVEN within the tolerance of the carried vector, and where nothing is forgotten the pass is serial and
//                exact.  Behind a chunk that was not walked the carried vector IS row c of `ends`, so the test there is
//                the one that opened the gate: it is made for 256 chunks at a time, a thread per chunk, and the walk jumps
//                from one chunk that failed it to the next (a scan of every boundary by one workgroup cost 50 ms at 4e4
//                chunks); only behind a chunk it has walked does it test the next start against the true vector.
//                diag[0] counts the chunks whose start did not stand against the replay's own end of the chunk before
//                (what opened the gate), diag[1] the chunks walked.
__global__ __launch_bounds__(kWalkThreads) void walk_kernel(const double* __restrict__ rho_tm, const double* __restrict__ a, int K,
                                                            int Kp, int64_t T, int64_t L, int64_t n_chunks,
                                                            const double* __restrict__ starts, const double* __restrict__ ends,
                                                            int force, double tol, const int* __restrict__ gate,
                                                            double* __restrict__ phi_tm, double* __restrict__ s_arr,
                                                            int64_t* __restrict__ diag) {
    if (!force && *gate == 0) return;
    __shared__ double cur[kWalkThreads];
    __shared__ double red[4];
    __shared__ unsigned long long masks[kWalkThreads / 64];
    const int tid = threadIdx.x;
    const bool state = tid < K;
    const int pos = hmm_pos(tid < Kp ? tid : 0);

    auto walk = [&](int64_t c) {                       // chunk c from cur; leaves its end in cur
        const int64_t t_lo = 1 + c * L, t_hi = t_lo + L < T ? t_lo + L : T;
        for (int64_t t = t_lo; t < t_hi; ++t) {
            double w = 0.0;
            if (state)
                for (int j = 0; j < K; ++j) w = fma(cur[j], a[(int64_t)j * K + tid], w);
            const double v = state ? w * rho_tm[t * Kp + pos] : 0.0;
            const double s = block_sum_256(v, red);      // (its barrier: every thread has read cur)
            const double phi = s > 0.0 ? v / s : 0.0;
            cur[tid] = phi;
            if (tid < Kp) phi_tm[t * Kp + pos] = phi;
            if (tid == 0) s_arr[t] = s;
            __syncthreads();
        }
    };

    if (force) {
        cur[tid] = state ? starts[tid] : 0.0;
        __syncthreads();
        for (int64_t c = 0; c < n_chunks; ++c) walk(c);
        return;
    }
    int64_t failed = 0, walked = 0;
    int64_t next = 1;                                  // chunks below it are settled
    int64_t proven = -1;                               // the chunk whose start stood against the TRUE vector behind a walk
    for (int64_t c0 = 1; c0 < n_chunks; c0 += kWalkThreads) {
        const int64_t mine = c0 + tid;
        bool bad = false;
        if (mine < n_chunks)
            for (int k = 0; k < K; ++k) bad = bad || entries_differ(starts[mine * Kp + k], ends[mine * Kp + k], tol);
        const unsigned long long ballot = __builtin_amdgcn_ballot_w64(bad);
        if ((tid & 63) == 0) masks[tid >> 6] = ballot;
        __syncthreads();
        for (int w = 0; w < kWalkThreads / 64; ++w) {
            unsigned long long m = masks[w];
            failed += __builtin_popcountll(m);
            while (m != 0ull) {
                const int64_t f = c0 + 64 * w + __builtin_ctzll(m);
                m &= m - 1ull;
                if (f < next || f == proven) continue;
                // chunks next .. f - 1 stand, each against the recorded end before it: the carried vector is row f of `ends`
                __syncthreads();
                cur[tid] = state ? ends[f * Kp + tid] : 0.0;
                __syncthreads();
                int64_t c = f;
                bool again;
                do {
                    walk(c);
                    ++walked;
                    ++c;
                    again = c < n_chunks && __syncthreads_or(state && entries_differ(starts[c * Kp + tid], cur[tid], tol)) != 0;
                } while (again);
                next = c;
                proven = c;
            }
        }
        __syncthreads();                               // (masks are rewritten by the next round)
    }
    if (tid == 0) {
        diag[0] = failed;
        diag[1] = walked;
    }
}

// ln p_t = ln s_t + m_t; z_t = the first maximum of phi_t in natural state order; end = phi_{T-1} in natural order.
__global__ __launch_bounds__(256) void close_kernel(const double* __restrict__ phi_tm, const double* __restrict__ s_arr,
                                                    const double* __restrict__ mx, int K, int Kp, int64_t T,
                                                    double* __restrict__ lnp, int64_t* __restrict__ z, double* __restrict__ end) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < T) {
        lnp[t] = log(s_arr[t]) + mx[t];
        if (z != nullptr) {
            const double* row = phi_tm + t * Kp;
            double best = row[0];                        // (state 0 is position 0)
            int arg = 0;
            for (int k = 1; k < K; ++k) {
                const double v = row[hmm_pos(k)];
                if (v > best) {
                    best = v;
                    arg = k;
                }
            }
            z[t] = arg;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < K) end[threadIdx.x] = phi_tm[(T - 1) * Kp + hmm_pos(threadIdx.x)];
}

}  // namespace hmmpred
