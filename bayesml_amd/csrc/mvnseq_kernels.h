// Kernels of sequential prediction for the Gauss-Wishart model of multivariate_normal (include/mvnseq.h; derivation in
// DESIGN.md 4f, "Sequential prediction, multivariate normal").  With S = hn_w_mat_inv, kappa_i = kappa_0 + i and the
// innovation u_i = sqrt(kappa_i / (kappa_i + 1)) (x_i - m_i), S_{i+1} = S_i + u_i u_i^T: the start matrix plus a plain Gram
// matrix of innovation rows, regression's Lambda = Lambda_0 + sum w w^T with w := u.  The schedule, the Gram body, the
// blocked factorisation and the double-double factor are regseq_kernels.h's; a pass over a range of blocks is
//
// (0) regseq::block_table_kernel: the rows [table[b], table[b + 1]) of the pass's blocks.
// (1) block_colsum_kernel: per block, the column sums of x - pivot in row order (pivot = row 0 of the call's x).
// (2) colsum_scan_kernel: one thread per column walks the blocks in order from carry's sum, leaving every block's
//     exclusive prefix in place of its sum and the total in carry.
// (3) block_means_kernel: per row, m_i - pivot = (kappa_0 (m_0 - pivot) + (block-start sum + in-block exclusive prefix)) /
//     kappa_i into the pass-sized scratch mean_rel [rows of the pass][D], c_i = sqrt(kappa_i / (kappa_i + 1)) into
//     scale [rows of the pass], and pivot + that to p_m where the caller asks for the means.
// (4) regseq::block_gram_kernel over CentredRows: value(n, f) = c_n ((x - pivot) - mean_rel[n][f]); U is never made.
// (5) gram_scan_kernel: the block Grams' exclusive prefix from carry, elementwise and in block order, into the state areas.
// (6) block_start_kernel: S_c = S_0 + G = L L^T on the state area, sum ln diag L, the factor inverted in place.
//     State area:  [ L^-1 [PD][PD] | unused [PD] | sum_j ln L_jj | unused ].
// (7) block_innovations_kernel: Z = U L^-T in sixteen-column slices on v_mfma_f64_16x16x4_f64, K = I + Z Z^T = R R^T (the
//     ten lower tiles in accumulators, the 64 x 64 factorisation in LDS; in double-double for a block of the first 2 D
//     rows or with a diagonal entry of K above regseq::kDdThreshold), then per row i of the block
//         q_i = u_i^T S_i^-1 u_i = z_i . z_i - sum_{j < i} R_ij^2      (= R_ii^2 - 1, without the cancellation against 1)
//         ln det S_i = 2 sum ln diag L + sum_{j < i in block} log1p(q_j)
//         p_nu = nu_i - D + 1,  ln det p_v_mat = D ln(kappa_i p_nu / (kappa_i + 1)) - ln det S_i,  quad = p_nu q_i,
//         nats = lnGamma(p_nu / 2) - lnGamma((p_nu + D) / 2) + (D / 2) ln(pi p_nu) - ln det p_v_mat / 2
//                + ((p_nu + D) / 2) log1p(q_i).
// No atomics, no waiting on other workgroups, every sum in a fixed order: one pass or many add the same numbers.
#pragma once
#include "regseq_kernels.h"

namespace mvnseq {
using gmmvb::d4;
using gmmvb::mfma_f64;
using gmmvb::sum_wave;
using regseq::dd;
using regseq::kBlock;
using regseq::kKLd;
using regseq::kTriLen;
using regseq::kTriPerThread;
using regseq::kZLd;
using regseq::padded;
using regseq::state_len;
using regseq::tri_at;

// ---- the row source of (4) and (7): the innovation rows, formed where they are read --------------------------------------
// (interface of regvb::MatrixRows: raw() is a plain load from an always valid address, value() what the element is)
template <typename XT>
struct CentredRows {
    typedef XT raw_t;
    typedef float target_t;
    const XT* x;
    int64_t ldx;
    int D;
    const double* mean_rel;      // [rows of the pass][D]
    const double* scale;         // [rows of the pass]
    int64_t row0;                // first row of the pass
    __device__ __forceinline__ XT raw(int64_t n, int f) const { return x[n * ldx + (f < D ? f : D - 1)]; }
    __device__ __forceinline__ double value(int64_t n, int f, XT v) const {
        const int fc = f < D ? f : D - 1;
        const int64_t r = n - row0;
        const double u = scale[r] * (((double)v - (double)x[fc]) - mean_rel[r * D + fc]);
        return f < D ? u : 0.0;
    }
    __device__ __forceinline__ float raw_target(int64_t) const { return 0.0f; }      // (the Gram body's c and s stay zero)
};

// ---- (1) -----------------------------------------------------------------------------------------------------------------
template <typename XT>
__global__ __launch_bounds__(256) void block_colsum_kernel(const XT* __restrict__ x, int64_t ldx, int D,
                                                           const int64_t* __restrict__ table,
                                                           double* __restrict__ colsum /*[nb][PD]*/) {
    const int f = threadIdx.x;
    if (f >= D) return;
    const int64_t lo = table[blockIdx.x], hi = table[blockIdx.x + 1];
    const double pivot = (double)x[f];
    double a = 0.0;
    for (int64_t r = lo; r < hi; ++r) a += (double)x[r * ldx + f] - pivot;
    colsum[(int64_t)blockIdx.x * padded(D) + f] = a;
}

// ---- (2) -----------------------------------------------------------------------------------------------------------------
static __global__ void colsum_scan_kernel(int64_t nb, int D, double* __restrict__ carry /*[D D + D + 1]*/,
                                          double* __restrict__ colsum) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= D) return;
    const int PD = padded(D);
    double run = carry[(int64_t)D * D + f];
    for (int64_t b = 0; b < nb; ++b) {
        const double t = colsum[b * PD + f];
        colsum[b * PD + f] = run;
        run += t;
    }
    carry[(int64_t)D * D + f] = run;
}

// ---- (3) -----------------------------------------------------------------------------------------------------------------
template <typename XT>
__global__ __launch_bounds__(256) void block_means_kernel(const XT* __restrict__ x, int64_t ldx, int D,
                                                          const int64_t* __restrict__ table,
                                                          const double* __restrict__ start /*[D D + D + 2]*/,
                                                          const double* __restrict__ colsum, double* __restrict__ mean_rel,
                                                          double* __restrict__ scale, double* __restrict__ p_m,
                                                          int64_t ld_pm) {
    const int f = threadIdx.x;
    if (f >= D) return;
    const int64_t lo = table[blockIdx.x], hi = table[blockIdx.x + 1], row0 = table[0];
    const double kappa0 = start[(int64_t)D * D + D];
    const double pivot = (double)x[f];
    const double base = kappa0 * (start[(int64_t)D * D + f] - pivot);
    const double before = colsum[(int64_t)blockIdx.x * padded(D) + f];
    double in = 0.0;               // the block's rows before r, in row order
    for (int64_t r = lo; r < hi; ++r) {
        const double kappa = kappa0 + (double)r;
        const double m = (base + (before + in)) / kappa;
        mean_rel[(r - row0) * D + f] = m;
        if (p_m) p_m[r * ld_pm + f] = pivot + m;
        if (f == 0) scale[r - row0] = sqrt(kappa / (kappa + 1.0));
        in += (double)x[r * ldx + f] - pivot;
    }
}

// ---- (5) -----------------------------------------------------------------------------------------------------------------
// (slab position of an element of G: regseq::block_scan_kernel's, the upper one of two mirror elements)
static __global__ void gram_scan_kernel(const double* __restrict__ slabs, const int64_t* __restrict__ table, int64_t nb,
                                        int T, int D, double* __restrict__ carry, double* __restrict__ states) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t dd = (int64_t)D * D;
    if (e > dd) return;
    if (e == dd) {                 // the row count: exact in binary64
        carry[dd + D] += (double)(table[nb] - table[0]);
        return;
    }
    const int PD = padded(D);
    const int64_t slab = regvb::gram_slab_len(T), ss = state_len(D);
    int u = (int)(e / D), w = (int)(e % D);
    const int64_t pos = (int64_t)u * PD + w;
    if (u > w) {
        const int t = u;
        u = w;
        w = t;
    }
    const int t1 = u >> 4, t2 = w >> 4, m = u & 15;
    const int64_t idx = ((int64_t)gmmvb::pair_index(t2, t1) * 4 + (m >> 2)) * 64 + (m & 3) * 16 + (w & 15);
    double run = carry[e];
    for (int64_t b = 0; b < nb; ++b) {
        const double t = slabs[b * slab + idx];
        states[b * ss + pos] = run;
        run += t;
    }
    carry[e] = run;
}

// ---- (6) -----------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(1024) void block_start_kernel(const double* __restrict__ start, int D, double* states) {
    __shared__ double dinv[16 * gmmvb::kDinvSize];
    const int PD = padded(D), ntl = PD >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* mat = states + (int64_t)blockIdx.x * state_len(D);
    double* tail = mat + (int64_t)PD * PD;
    for (int e = tid; e < PD * PD; e += 1024) {
        const int i = e / PD, j = e - i * PD;
        mat[e] = (i < D && j < D) ? (j <= i ? start[(int64_t)i * D + j] + mat[e] : 0.0) : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    gmmvb::blocked_cholesky<16, true>(mat, PD, ntl, dinv);
    __syncthreads();
    if (wv == 0) {                 // sum ln diag L before the factor is inverted in place: lane-strided, then across the wave
        double a = 0.0;
        for (int j = lane; j < D; j += 64) a += log(mat[j * PD + j]);
        a = sum_wave(a);
        if (lane == 0) tail[PD] = a;
    }
    __syncthreads();
    gmmvb::blocked_tri_inverse_subst<16>(mat, PD, ntl, dinv);
}

// ---- (7) -----------------------------------------------------------------------------------------------------------------
// lnGamma(a) - lnGamma(a + h), h = D / 2: from a = 64 on the difference of the two Stirling series (the lgamma values
// agree in their leading digits there), lnGamma(a + h) - lnGamma(a) = (a - 1/2) log1p(h / a) + h ln(a + h) - h + t(a + h) - t(a)
__device__ __attribute__((noinline)) double lgamma_step(double a, double h) {
    if (a < 64.0) return lgamma(a) - lgamma(a + h);
    return -((a - 0.5) * log1p(h / a) + h * log(a + h) - h + (regseq::stirling_tail(a + h) - regseq::stirling_tail(a)));
}

struct RowOutputs {
    double* logdet;
    double* quad;
    double* nats;      // each [n_rows] or null
};

// The slices, K and its factorisation are regseq::block_innovations_kernel's, restated so that that kernel's code stays
// as it is; what follows the factorisation is this model's.
template <typename SRC>
__global__ __launch_bounds__(256) void block_innovations_kernel(SRC src, const int64_t* __restrict__ table,
                                                                const double* __restrict__ states,
                                                                const double* __restrict__ start, int D, RowOutputs out) {
    static_assert(kBlock == 64, "four waves of 16 rows; the closing formulas are one wave with lane = row");
    __shared__ double km[kBlock * kKLd];
    __shared__ double zs[2 * kBlock * kZLd];
    __shared__ double dinv[(kBlock / 16) * gmmvb::kDinvSize];
    __shared__ double szz[kBlock], sl[kBlock];
    const int PD = padded(D), nt = PD >> 4;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t lo = table[blockIdx.x], hi = table[blockIdx.x + 1];
    const double* mat = states + (int64_t)blockIdx.x * state_len(D);
    const int64_t row = lo + 16 * wv + li;
    const bool valid = row < hi;
    const int64_t rowc = valid ? row : hi - 1;
    for (int e = tid; e < kBlock * kKLd; e += 256) km[e] = 0.0;
    // K and its factor in double-double: a block of the first 2 D rows of the call, or, decided after the binary64 slices,
    // one whose K has a diagonal entry above the threshold.  Workgroup uniform, a function of the block's rows and start state.
    bool head = lo < 2 * (int64_t)D;
    dd kd[kTriPerThread];
    int ki[kTriPerThread], kj[kTriPerThread];
    d4 kacc[3];        // the wave's lower tiles of K: numbers wv, wv + 4, wv + 8 of (0,0) (1,0) (1,1) (2,0) ... (3,3)
#pragma unroll
    for (int k = 0; k < 3; ++k) kacc[k] = d4{0.0, 0.0, 0.0, 0.0};
    for (;;) {
#pragma unroll
        for (int k = 0; k < kTriPerThread; ++k) {
            ki[k] = kj[k] = 0;
            kd[k] = dd{0.0, 0.0};
            if (head) {
                const int e = tid + 256 * k < kTriLen ? tid + 256 * k : kTriLen - 1;
                int i = 0;
                while (tri_at(i + 1, 0) <= e) ++i;
                ki[k] = i;
                kj[k] = e - tri_at(i, 0);
                kd[k].hi = i == kj[k] ? 1.0 : 0.0;
            }
        }
        for (int s = 0; s < nt; ++s) {
            d4 z = d4{0.0, 0.0, 0.0, 0.0};
            for (int jt = 0; jt <= s; ++jt) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int f = 16 * jt + 4 * p + lg;                         // (f < PD: the source clamps it)
                    const double a = valid ? src.value(rowc, f, src.raw(rowc, f)) : 0.0;
                    z = mfma_f64(a, mat[(16 * s + li) * PD + f], z);
                }
            }
            double* buf = zs + (s & 1) * (kBlock * kZLd);
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[(16 * wv + lg + 4 * r) * kZLd + li] = z[r];
            __syncthreads();           // (buffer s & 1 is written again at s + 2, behind the barrier of s + 1)
            if (head) {
#pragma unroll
                for (int k = 0; k < kTriPerThread; ++k)
                    for (int c = 0; c < 16; ++c)
                        kd[k] = regseq::dd_add(kd[k], regseq::dd_two_prod(buf[ki[k] * kZLd + c], buf[kj[k] * kZLd + c]));
                continue;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int t = wv + 4 * k;
                if (t < 10) {
                    const int rt = t >= 6 ? 3 : (t >= 3 ? 2 : (t >= 1 ? 1 : 0)), ct = t - rt * (rt + 1) / 2;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        kacc[k] = mfma_f64(buf[(16 * rt + li) * kZLd + 4 * p + lg], buf[(16 * ct + li) * kZLd + 4 * p + lg], kacc[k]);
                }
            }
        }
        if (head) break;
        bool large = false;            // the largest diagonal entry of the binary64 K (diagonal tiles 0, 2, 5, 9)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = wv + 4 * k;
            if (t == 0 || t == 2 || t == 5 || t == 9) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (lg + 4 * r == li) large = large || kacc[k][r] + 1.0 > regseq::kDdThreshold;
            }
        }
        if (!__syncthreads_or(large)) break;
        head = true;
    }
    __syncthreads();               // km is zero everywhere
    if (head) {
#pragma unroll
        for (int k = 0; k < kTriPerThread; ++k)
            if (tid + 256 * k < kTriLen) {
                km[tid + 256 * k] = kd[k].hi;
                km[kTriLen + tid + 256 * k] = kd[k].lo;
            }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = wv + 4 * k;
            if (t < 10) {
                const int rt = t >= 6 ? 3 : (t >= 3 ? 2 : (t >= 1 ? 1 : 0)), ct = t - rt * (rt + 1) / 2;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * rt + lg + 4 * r, j = 16 * ct + li;
                    if (j <= i) km[i * kKLd + j] = kacc[k][r] + (i == j ? 1.0 : 0.0);
                    if (j == i) szz[i] = kacc[k][r];           // z_i . z_i, before the one is added
                }
            }
        }
    }
    __syncthreads();
    if (head)
        regseq::dd_cholesky_packed(km, km + kTriLen);
    else
        gmmvb::blocked_cholesky<kBlock / 16>(km, kKLd, kBlock / 16, dinv);
    if (wv != 0) return;
    // q_i, lane = row: R_ii^2 - 1 in double-double where the factor is; z_i . z_i - sum_{j < i} R_ij^2 in binary64 otherwise
    double q;
    if (head) {
        const dd r = dd{km[tri_at(lane, lane)], km[kTriLen + tri_at(lane, lane)]};
        q = regseq::dd_add(regseq::dd_mul(r, r), dd{-1.0, 0.0}).hi;
    } else {
        double s = 0.0;
        for (int j = 0; j < kBlock - 1; ++j)
            if (j < lane) s = fma(km[lane * kKLd + j], km[lane * kKLd + j], s);
        q = szz[lane] - s;
    }
    q = fmax(q, 0.0);
    const double l = log1p(q);         // ln(R_ii^2)
    sl[lane] = l;
    __builtin_amdgcn_wave_barrier();
    double before = 0.0;               // sum of ln(R_jj^2) over the block's earlier rows, in row order
    for (int j = 0; j < kBlock - 1; ++j)
        if (j < lane) before += sl[j];
    const int64_t i = lo + lane;
    if (i >= hi) return;
    const double kappa = start[(int64_t)D * D + D] + (double)i;
    const double p_nu = ((start[(int64_t)D * D + D + 1] + (double)i) - (double)D) + 1.0;
    const double logdet_s = 2.0 * mat[(int64_t)PD * PD + PD] + before;
    const double logdet_v = (double)D * log(kappa * p_nu / (kappa + 1.0)) - logdet_s;
    const double h = 0.5 * (double)D;
    if (out.logdet) out.logdet[i] = logdet_v;
    if (out.quad) out.quad[i] = p_nu * q;
    if (out.nats)
        out.nats[i] = lgamma_step(0.5 * p_nu, h) + h * log(3.141592653589793238 * p_nu) - 0.5 * logdet_v
                      + (0.5 * p_nu + h) * l;
}

}  // namespace mvnseq
