// Student-t mixture log-density: ln p_i = logsumexp_k [ c_k - a_k log1p(q_ik / nu_k) ], q_ik = || U_k (x_i - mu_k) ||^2.
//
// The quadratic forms are the dense E-step's (estep.h: same parameter image, same wave tile, same f64 MFMA product with the
// upper tile pairs skipped, component images double-buffered into LDS by global_load_lds); what follows them is this
// file's: q stays in registers, and every row carries a running maximum M, a running sum s of exp(t - M) and the first
// arg-max through the k loop (online log-sum-exp), so one value per row is stored instead of K.
//
// Pivot: the image's bias block is -U_k (mu_k - pivot) (pack_kernel below), and the kernels subtract the same pivot from a
// row as they widen it to binary64 - the rows of a wave tile are held centred, as doubles, whatever their storage, so
// the wave tile is the f64 E-step's for f32 rows too.  The lane's 4 T pivot entries are read with the tile's rows and die
// with them: kept across the k loop they are 8 T more registers, which at T = 8 no longer fit beside the accumulators.
//
// D > 128: plain_kernel, the same formulas on the vector ALU with U_k read through scalar loads (generic.h's scheme).
#pragma once
#include "aux_kernels.h"
#include "estep.h"
#include "generic.h"

namespace stmix {

using gmmvb::d4;
using gmmvb::estep_kb;
using gmmvb::estep_nb_w;
using gmmvb::img_doubles;

constexpr int kWaves = 8;          // two waves per SIMD: one's closing (log1p, exp on the vector ALU) under the other's MFMAs

// doubles per component of the image
__host__ __device__ constexpr int64_t image_doubles(int D) {
    return D <= 128 ? (int64_t)img_doubles((D + 15) / 16) : (int64_t)D * D + D;
}

// ---- the image -----------------------------------------------------------------------------------------------------------
// One workgroup per component: d = mu_k - pivot, then the E-step's image of (U_k, d) (D <= 128) or [U_k | -U_k d] (D > 128,
// the bias by the same ascending fma chain as pack_f64_image's).
static __global__ __launch_bounds__(256) void pack_kernel(const double* __restrict__ u, const double* __restrict__ m,
                                                          const double* __restrict__ pivot, int D,
                                                          double* __restrict__ img) {
    __shared__ double d[128];
    const int k = blockIdx.x;
    const double* uk = u + (int64_t)k * D * D;
    const double* mk = m + (int64_t)k * D;
    double* out = img + (int64_t)k * image_doubles(D);
    if (D <= 128) {
        for (int i = threadIdx.x; i < D; i += blockDim.x) d[i] = mk[i] - pivot[i];
        __syncthreads();
        const int T = (D + 15) / 16;
        gmmvb::pack_f64_image(uk, D, d, D, T, img_doubles(T), out);
        return;
    }
    for (int64_t e = threadIdx.x; e < (int64_t)D * D; e += blockDim.x) {
        const int j = (int)(e / D), i = (int)(e - (int64_t)j * D);
        out[e] = i <= j ? uk[e] : 0.0;
    }
    for (int j = threadIdx.x; j < D; j += blockDim.x) {
        double s = 0.0;
        for (int i = 0; i <= j; ++i) s = fma(uk[(int64_t)j * D + i], mk[i] - pivot[i], s);
        out[(int64_t)D * D + j] = -s;
    }
}

// ---- the closing ---------------------------------------------------------------------------------------------------------
// One (row, component) pair into the row's running log-sum-exp: after the call M = max t so far, s = sum exp(t - M), z = the
// first k at which the maximum was reached.  One exp per pair; t = -inf (a weight of zero) adds nothing; a NaN stays.
__device__ __forceinline__ void close_pair(double q, double c, double nu, double a, int k, double& M, double& s, int& z) {
    const double t = c - a * log1p(q / nu);
    const double d = t - M;
    const double e = t == -__builtin_huge_val() ? 0.0 : exp(-fabs(d));
    if (d > 0.0) {
        s = s * e + 1.0;
        M = t;
        z = k;
    } else {
        s += e;
    }
}
__device__ __forceinline__ double close_row(double M, double s) { return M + log(s); }

// ---- D <= 128 ------------------------------------------------------------------------------------------------------------
// estep_component (estep.h) with the values returned instead of stored: q[nb] = || U_k xc + bias ||^2 of this lane's rows,
// summed over the lane groups (every lane of a row gets it).  Same operations in the same order.
template <int NB, int T, typename ImgPtr>
__device__ __forceinline__ void quad_component(ImgPtr im, const double (&xc)[NB][T][4], int lane, int g, double (&q)[NB]) {
    constexpr int P = gmmvb::tri_pairs(T);
    typedef double d2 __attribute__((ext_vector_type(2)));
    d4 acc[T][NB];
#pragma unroll
    for (int jt = 0; jt < T; ++jt) {
        const d2 b01 = *reinterpret_cast<const d2*>(im + P * 256 + (jt * 4 + g) * 4);
        const d2 b23 = *reinterpret_cast<const d2*>(im + P * 256 + (jt * 4 + g) * 4 + 2);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[jt][nb] = d4{b01[0], b01[1], b23[0], b23[1]};
    }
#pragma unroll
    for (int jt = 0; jt < T; ++jt) {
#pragma unroll
        for (int b = 0; b <= jt; ++b) {
            const int p = gmmvb::pair_index(jt, b);
            const d2 a01 = *reinterpret_cast<const d2*>(im + p * 256 + lane * 2);
            const d2 a23 = *reinterpret_cast<const d2*>(im + p * 256 + 128 + lane * 2);
            const double a[4] = {a01[0], a01[1], a23[0], a23[1]};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[jt][nb] = gmmvb::mfma_f64(a[s], xc[nb][b][s], acc[jt][nb]);
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        double v = 0.0;
#pragma unroll
        for (int jt = 0; jt < T; ++jt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v = fma(acc[jt][nb][r], acc[jt][nb][r], v);
        }
        q[nb] = gmmvb::sum_groups(v);
    }
}

// estep_lds_f64's structure (estep.h).  lnp [n_rows], z [n_rows] or null: only the g == 0 lanes store, rows past n_rows are
// clamped on load and masked on store.
template <int T, typename XT, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void fused_kernel(const XT* __restrict__ x, int64_t ldx, int64_t n_rows, int D,
                                                            const double* __restrict__ pivot,
                                                            const double* __restrict__ img /*[K][IMG]*/,
                                                            const double* __restrict__ cvec, const double* __restrict__ nuvec,
                                                            int K, double* __restrict__ lnp, int64_t* __restrict__ z) {
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

    // global -> LDS copy of component block kb: 1-KB pieces (64 lanes x 16 B), lane-linear on both sides
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
                    const double pv = f < D ? pivot[f] : 0.0;      // (the lane's 4 T pivot entries)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) xc[nb][b][s] = (double)xr[nb][b][s] - pv;
                }
            }
        }
        double M[NB], S[NB];
        int Z[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            M[nb] = -__builtin_huge_val();
            S[nb] = 0.0;
            Z[nb] = 0;
        }
        stage(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kb = 0; kb < n_blocks; ++kb) {
            if (kb + 1 < n_blocks) stage(kb + 1, (kb + 1) & 1);      // prefetch a whole block ahead
            const double* buf = smem[kb & 1];
            const int k0 = kb * KB;
#pragma unroll 1
            for (int kk = 0; kk < KB; ++kk) {
                const int k = k0 + kk;
                if (k >= K) break;
                double q[NB];
                quad_component<NB, T>(buf + kk * IMG, xc, lane, g, q);
                const double c = cvec[k], nu = nuvec[k];
                const double a = 0.5 * (nu + dims);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) close_pair(q[nb], c, nu, a, k, M[nb], S[nb], Z[nb]);
            }
            // the prefetched block must have landed, and every wave must be done reading this one
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            if (g == 0 && stv[nb] >= 0) {
                lnp[stv[nb]] = close_row(M[nb], S[nb]);
                if (z) z[stv[nb]] = Z[nb];
            }
        }
    }
}

// ---- D > 128 -------------------------------------------------------------------------------------------------------------
// One wave per R = generic_rows(D) rows, a lane per row, the centred rows in LDS feature-major; the k loop runs inside the
// kernel in the fused kernel's order, so the first-maximum rule is the same.  U_k[j][i] and the bias come through scalar
// loads (the address does not depend on the lane).
template <typename XT>
__global__ __launch_bounds__(64) void plain_kernel(const XT* __restrict__ x, int64_t ldx, int64_t n_rows, int D,
                                                   const double* __restrict__ pivot, const double* __restrict__ img,
                                                   const double* __restrict__ cvec, const double* __restrict__ nuvec, int K,
                                                   int R, double* __restrict__ lnp, int64_t* __restrict__ z) {
    extern __shared__ double dsh[];                           // [D][R]
    const int lane = threadIdx.x;
    const int col = lane < R ? lane : 0;
    const int64_t n_tiles = (n_rows + R - 1) / R;
    const double dims = (double)D;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile * R + lane;
        const bool live = lane < R && row < n_rows;
        __syncthreads();                                      // the previous tile's rows have been read
        if (lane < R) {
            const XT* xr = x + (live ? row : n_rows - 1) * ldx;
            for (int i = 0; i < D; ++i) dsh[(int64_t)i * R + lane] = (double)xr[i] - pivot[i];
        }
        __syncthreads();
        double M = -__builtin_huge_val(), S = 0.0;
        int Z = 0;
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
            close_pair(q, cvec[k], nu, 0.5 * (nu + dims), k, M, S, Z);
        }
        if (live) {
            lnp[row] = close_row(M, S);
            if (z) z[row] = Z;
        }
    }
}

}  // namespace stmix
