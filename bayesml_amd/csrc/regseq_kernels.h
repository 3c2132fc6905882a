// Kernels of sequential prediction for the Normal-Gamma regression family (include/regseq.h; derivation in DESIGN.md 4f,
// "Sequential prediction").  The rows of a call are cut into blocks (schedule below); a pass works on a range of them:
//
// (0) block_table_kernel: the rows [table[b], table[b + 1]) of the pass's blocks.  Every other kernel takes its bounds
//     from this table, so the ramp blocks and the cut last block need no launch of their own.
// (1) block_gram_kernel: regvb_kernels.h's gram_body over each block's rows, one workgroup and one slab per block, with the
//     same row sources (MatrixRows, WindowRows: the window matrix is never made).
// (2) block_scan_kernel: one thread per element of [G | c | s | n]; walks the blocks in order, prefix[b + 1] = prefix[b] +
//     block[b], starting from `carry` and leaving the total there: the additions of a call are the same whatever the passes.
//     Block b's prefix lands in its state area, G with row stride PD (D rounded up to 16).
// (3) block_start_kernel: one workgroup per block turns the prefix into the state at the block's first row: Lambda_c =
//     Lambda_0 + G is factorised and the factor inverted in place (chol_blocked.h, on the state area itself: at D = 256
//     the matrix is 0.5 MB, more than a CU's LDS; the workgroup's barriers order its own global accesses),
//     u = L^-1 (Lambda_0 mu_0 + c), mu_c = L^-T u (by substitution, before the inversion),
//     beta_c = beta_0 + (s + mu_0^T Lambda_0 mu_0 - |u|^2) / 2 (|u|^2 is mu_c^T Lambda_c mu_c).
//     State area:  [ L^-1 [PD][PD] | mu_c [PD] | beta_c | rows before the block ].
// (4) block_innovations_kernel: one workgroup (four waves, 16 rows each) per block of up to B = 64 rows W.  Z = W L^-T is
//     formed sixteen columns at a time on v_mfma_f64_16x16x4_f64 (rows and factor straight from memory: the slice of the
//     factor is read by all 256 CUs and stays in L2), each slice goes through LDS into K = I + Z Z^T, whose ten lower
//     16 x 16 tiles stay in the waves' accumulators; Z itself (128 KiB at D = 256) never exists.  Then K = R R^T in LDS
//     (blocked_cholesky), v = R^-1 (y - W mu_c) by forward substitution in one wave (lane = row), the in-block prefix of
//     v^2 in row order, and per row i
//         s = R_ii^2,  beta_i = beta_c + sum_{j < i} v_j^2 / 2,  alpha_i = alpha_0 + (rows before i) / 2,
//         p_lambda = alpha_i / (beta_i s),  p_nu = 2 alpha_i,  p_m = y_i - R_ii v_i,
//         nats = lnGamma(alpha_i) - lnGamma(alpha_i + 1/2) + ln(2 pi alpha_i / p_lambda) / 2 + (alpha_i + 1/2) log1p(v_i^2 / (2 beta_i)).
//     Rows past the block's end are zero rows (K = I there) and write nothing.  A block that starts within the first 2 D
//     rows of the call, or whose binary64 K turns out to have a diagonal entry above kDdThreshold (a regressor that
//     switches on late under a diffuse prior), forms K and factorises it in double-double on the vector ALU instead: the
//     latter runs its slices a second time (see "double-double" below).
// No atomics, no waiting on other workgroups, every sum in a fixed order.
#pragma once
#include "chol_blocked.h"
#include "regvb_kernels.h"

namespace regseq {
using gmmvb::d4;
using gmmvb::mfma_f64;
using gmmvb::sum_groups;
using gmmvb::sum_wave;

constexpr int kBlock = 64;           // include/regseq.h: REGSEQ_BLOCK
constexpr int kLog2Block = 6;
static_assert(1 << kLog2Block == kBlock, "the ramp doubles up to the block length");
constexpr int kZLd = 17, kKLd = kBlock + 1;

// ---- the schedule: blocks of 1, 2, 4, ..., B / 2 rows, then of B rows, the last one cut at n -----------------------------
__host__ __device__ inline int64_t block_count(int64_t n) {
    if (n < kBlock - 1) {
        int k = 0;
        while (((int64_t)1 << k) - 1 < n) ++k;
        return k;
    }
    return kLog2Block + (n - (kBlock - 1) + kBlock - 1) / kBlock;
}
__host__ __device__ inline int64_t block_start(int64_t n, int64_t b) {
    const int64_t r = b <= kLog2Block ? ((int64_t)1 << b) - 1 : kBlock - 1 + (b - kLog2Block) * kBlock;
    return r < n ? r : n;
}

__host__ __device__ constexpr int padded(int D) { return (D + 15) & ~15; }
// doubles of a block's state area
__host__ __device__ constexpr int64_t state_len(int D) { return (int64_t)padded(D) * padded(D) + padded(D) + 2; }

// ---- (0) -----------------------------------------------------------------------------------------------------------------
static __global__ void block_table_kernel(int64_t n, int64_t b0, int64_t nb, int64_t* __restrict__ table /*[nb + 1]*/) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= nb) table[i] = block_start(n, b0 + i);
}

// ---- (1) -----------------------------------------------------------------------------------------------------------------
template <int T, typename SRC>
__global__ __launch_bounds__(32 * T) void block_gram_kernel(SRC src, const int64_t* __restrict__ table,
                                                            double* __restrict__ slabs /*[nb][gram_slab_len(T)]*/) {
    __shared__ __attribute__((aligned(16))) double sx[2 * regvb::kBatch * 16 * T];
    __shared__ double sy[2 * regvb::kBatch];
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t lo = table[blockIdx.x], hi = table[blockIdx.x + 1];       // (hi > lo: the schedule has no empty block)
    double* out = slabs + (int64_t)blockIdx.x * regvb::gram_slab_len(T);
    regvb::gram_dispatch<T>(sub, src, lo, hi, out, sx, sy, std::make_integer_sequence<int, T / 2>{});
}

// ---- (2) -----------------------------------------------------------------------------------------------------------------
// (the slab position of element e of [G | c | s | n] is gram_reduce_kernel's: the upper one of two mirror elements)
static __global__ void block_scan_kernel(const double* __restrict__ slabs, int64_t nb, int T, int D,
                                         double* __restrict__ carry /*[D D + D + 2]*/, double* __restrict__ states) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t dd = (int64_t)D * D, len = dd + D + 2;
    if (e >= len) return;
    const int PD = padded(D);
    const int64_t slab = regvb::gram_slab_len(T), ss = state_len(D);
    const int P = gmmvb::tri_pairs(T);
    int64_t idx, pos;
    if (e < dd) {
        int u = (int)(e / D), w = (int)(e % D);
        pos = (int64_t)u * PD + w;
        if (u > w) {
            const int t = u;
            u = w;
            w = t;
        }
        const int t1 = u >> 4, t2 = w >> 4, m = u & 15;
        idx = ((int64_t)gmmvb::pair_index(t2, t1) * 4 + (m >> 2)) * 64 + (m & 3) * 16 + (w & 15);
    } else {
        const int64_t k = e - dd;
        idx = (int64_t)P * 256 + (k < D ? k : 16 * T + (k - D));
        pos = (int64_t)PD * PD + (k < D ? k : PD + (k - D));
    }
    double run = carry[e];
    for (int64_t b = 0; b < nb; ++b) {
        const double t = slabs[b * slab + idx];
        states[b * ss + pos] = run;
        run += t;
    }
    carry[e] = run;
}

// ---- (3) -----------------------------------------------------------------------------------------------------------------
// (static: mvnseq.hip includes this header too)
static __global__ __launch_bounds__(1024) void block_start_kernel(const double* __restrict__ start /*[D D + D + 3]*/, int D,
                                                                  double* states) {
    __shared__ double dinv[16 * gmmvb::kDinvSize];
    __shared__ double sr[256], su[256];
    __shared__ double s_uu;
    const int PD = padded(D), ntl = PD >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* mat = states + (int64_t)blockIdx.x * state_len(D);
    double* tail = mat + (int64_t)PD * PD;
    for (int e = tid; e < PD * PD; e += 1024) {
        const int i = e / PD, j = e - i * PD;
        mat[e] = (i < D && j < D) ? (j <= i ? start[(int64_t)i * D + j] + mat[e] : 0.0) : (i == j ? 1.0 : 0.0);
    }
    if (tid < 256) sr[tid] = tid < D ? start[(int64_t)D * D + tid] + tail[tid] : 0.0;
    const double s = tail[PD], rows_before = tail[PD + 1];
    __syncthreads();
    gmmvb::blocked_cholesky<16, true>(mat, PD, ntl, dinv);
    __syncthreads();
    // u = L^-1 r and mu_c = L^-T u by substitution on the factor itself, before it is inverted in place: one wave, and
    // both sweeps read L by rows.  (Through the explicit inverse mu_c loses more digits under a diffuse prior: DESIGN.md)
    if (wv == 0) {
        double uu = 0.0;
        for (int j = 0; j < D; ++j) {                   // u_j = (r_j - sum_{i < j} L_ji u_i) / L_jj
            double a = 0.0;
            for (int i = lane; i < j; i += 64) a = fma(mat[j * PD + i], su[i], a);
            a = sum_wave(a);
            const double uj = (sr[j] - a) / mat[j * PD + j];
            if (lane == 0) su[j] = uj;
            uu = fma(uj, uj, uu);
            __builtin_amdgcn_wave_barrier();
        }
        for (int j = D - 1; j >= 0; --j) {              // mu_j = t_j / L_jj, then t_i -= L_ji mu_j for i < j
            const double m = su[j] / mat[j * PD + j];
            for (int i = lane; i < j; i += 64) su[i] = fma(-mat[j * PD + i], m, su[i]);
            if (lane == 0) sr[j] = m;
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) s_uu = uu;
    }
    __syncthreads();
    gmmvb::blocked_tri_inverse_subst<16>(mat, PD, ntl, dinv);
    if (tid < PD) tail[tid] = tid < D ? sr[tid] : 0.0;
    __syncthreads();
    if (tid == 0) {
        const double m0 = start[(int64_t)D * D + D], beta0 = start[(int64_t)D * D + D + 2];
        tail[PD] = beta0 + ((s + m0) - s_uu) / 2.0;
        tail[PD + 1] = rows_before;
    }
}

// ---- (4) -----------------------------------------------------------------------------------------------------------------
// Stirling's tail: lnGamma(x) = (x - 1/2) ln x - x + ln(2 pi) / 2 + t(x); below 1e-19 of truncation error from x = 64 on
__device__ __forceinline__ double stirling_tail(double x) {
    const double r = 1.0 / x, r2 = r * r;
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))));
}
// lnGamma(a) - lnGamma(a + 1/2): from a = 64 on the difference of the two series (the lgamma values agree in their leading
// digits there), lnGamma(a + h) - lnGamma(a) = a log1p(h / a) + h ln a - h + t(a + h) - t(a) at h = 1/2
__device__ __attribute__((noinline)) double lgamma_half_step(double a) {
    if (a < 64.0) return lgamma(a) - lgamma(a + 0.5);
    return -(a * log1p(0.5 / a) + 0.5 * log(a) - 0.5 + (stirling_tail(a + 0.5) - stirling_tail(a)));
}

// ---- double-double, for the blocks that start from a nearly singular Lambda_c ----------------------------------------------
// Until a call has seen 2 D rows, a block may start from a nearly singular Lambda_c (a diffuse prior): K = I + Z Z^T then
// has entries of 1e6 and more whose Schur complements s_i are of order one, and every rounding of K or of its factor in
// binary64 costs s_i that many digits, where the row loop refactorises Lambda and loses none.  Later blocks do the same
// when a regressor that was zero so far switches on in them (a regime dummy, a level first seen at row 70): Lambda_c has
// kept the prior's precision in that direction however many rows came before.  So a block forms K and factorises it in
// double-double on the vector ALU (error-free products by fma, Knuth's two-sum) when it starts within the first 2 D rows,
// or when a diagonal entry of its binary64 K exceeds kDdThreshold: K_ii = 1 + w_i^T Lambda_c^-1 w_i is 1 to 6 in every
// block past 2 D rows of the tests' ordinary inputs and 1e6 in the onset blocks, and a block just below
// the threshold loses at most that factor, six bits, in binary64.  The rounding of Z itself is harmless, s_i being
// insensitive to relative perturbations of the rows of Z.
constexpr double kDdThreshold = 64.0;
struct dd {
    double hi, lo;
};
// (contraction is off inside them: a product fused into a neighbouring sum would break the error-free transformations)
__device__ __forceinline__ dd dd_sum(double a, double b) {           // a + b exactly
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
    dd s = dd_sum(a.hi, b.hi);
    s.lo += a.lo + b.lo;
    const double h = s.hi + s.lo;
    return dd{h, s.lo - (h - s.hi)};
}
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
#pragma clang fp contract(off)
    const double p = a.hi * b.hi;
    const double e = fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    const double h = p + e;
    return dd{h, e - (h - p)};
}
__device__ __forceinline__ dd dd_neg(dd a) { return dd{-a.hi, -a.lo}; }
__device__ __forceinline__ dd dd_two_prod(double a, double b) {      // a b exactly
#pragma clang fp contract(off)
    const double p = a * b;
    return dd{p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_div(dd a, dd b) {                    // two correction steps on the binary64 quotient
#pragma clang fp contract(off)
    const double q1 = a.hi / b.hi;
    dd r = dd_add(a, dd_neg(dd_mul(dd{q1, 0.0}, b)));
    const double q2 = r.hi / b.hi;
    r = dd_add(r, dd_neg(dd_mul(dd{q2, 0.0}, b)));
    const double q3 = r.hi / b.hi;
    return dd_add(dd_sum(q1, q2), dd{q3, 0.0});
}
__device__ __forceinline__ dd dd_sqrt(dd a) {                        // one Newton step on the binary64 root
#pragma clang fp contract(off)
    const double x = sqrt(a.hi);
    const dd r = dd_add(a, dd_neg(dd_mul(dd{x, 0.0}, dd{x, 0.0})));
    return dd_sum(x, r.hi / (2.0 * x));
}
// position of (i, j), j <= i, in the packed lower triangle
__device__ __forceinline__ int tri_at(int i, int j) { return i * (i + 1) / 2 + j; }
constexpr int kTriLen = kBlock * (kBlock + 1) / 2;
static_assert(2 * kTriLen == kBlock * kKLd, "the packed hi and lo triangles take the place of the padded square");
constexpr int kTriPerThread = (kTriLen + 255) / 256;

// K = R R^T in double-double on the packed triangles khi | klo, 256 threads: column by column, right-looking, the
// trailing update on a 16 x 16 thread grid.  Leaves R in place.
__device__ __forceinline__ void dd_cholesky_packed(double* khi, double* klo) {
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    for (int j = 0; j < kBlock; ++j) {
        __syncthreads();
        const int jj = tri_at(j, j);
        const dd d = dd_sqrt(dd{khi[jj], klo[jj]});
        for (int i = j + 1 + tid; i < kBlock; i += 256) {
            const int e = tri_at(i, j);
            const dd x = dd_div(dd{khi[e], klo[e]}, d);
            khi[e] = x.hi;
            klo[e] = x.lo;
        }
        __syncthreads();
        if (tid == 0) {
            khi[jj] = d.hi;
            klo[jj] = d.lo;
        }
        for (int i = j + 1 + ti; i < kBlock; i += 16) {
            const int ei = tri_at(i, j);
            const dd rij = dd{-khi[ei], -klo[ei]};
            for (int k = j + 1 + tj; k <= i; k += 16) {
                const int ek = tri_at(k, j), e = tri_at(i, k);
                const dd x = dd_add(dd{khi[e], klo[e]}, dd_mul(rij, dd{khi[ek], klo[ek]}));
                khi[e] = x.hi;
                klo[e] = x.lo;
            }
        }
    }
    __syncthreads();
}

struct RowOutputs {
    double* p_m;
    double* p_lambda;
    double* p_nu;
    double* nats;      // each [n_rows] or null
};

template <typename SRC>
__global__ __launch_bounds__(256) void block_innovations_kernel(SRC src, const int64_t* __restrict__ table,
                                                                const double* __restrict__ states,
                                                                const double* __restrict__ start, int D, RowOutputs out) {
    static_assert(kBlock == 64, "four waves of 16 rows; the substitution is one wave with lane = row");
    __shared__ double km[kBlock * kKLd];
    __shared__ double zs[2 * kBlock * kZLd];
    __shared__ double dinv[(kBlock / 16) * gmmvb::kDinvSize];
    __shared__ double se[kBlock], sy[kBlock], sv2[kBlock];
    const int PD = padded(D), nt = PD >> 4;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t lo = table[blockIdx.x], hi = table[blockIdx.x + 1];
    const double* mat = states + (int64_t)blockIdx.x * state_len(D);
    const double* mu = mat + (int64_t)PD * PD;
    const int64_t row = lo + 16 * wv + li;
    const bool valid = row < hi;
    const int64_t rowc = valid ? row : hi - 1;
    for (int e = tid; e < kBlock * kKLd; e += 256) km[e] = 0.0;
    // K and its factor in double-double (above): a block of the first 2 D rows of the call, or, decided after the binary64
    // slices below, one whose K has a diagonal entry above kDdThreshold.  Workgroup uniform, and a function of the
    // block's rows and start state alone.  The thread's entries of the packed triangle are tid, tid + 256, ...
    bool head = mu[PD + 1] < 2.0 * D;
    dd kd[kTriPerThread];
    int ki[kTriPerThread], kj[kTriPerThread];
    // the wave's lower tiles of K: numbers wv, wv + 4, wv + 8 of (0,0) (1,0) (1,1) (2,0) ... (3,3)
    d4 kacc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) kacc[k] = d4{0.0, 0.0, 0.0, 0.0};
    double dot;
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
        dot = 0.0;
        for (int s = 0; s < nt; ++s) {
            d4 z = d4{0.0, 0.0, 0.0, 0.0};
            for (int jt = 0; jt <= s; ++jt) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int f = 16 * jt + 4 * p + lg;                         // (f < PD <= 16 T: the sources clamp it)
                    const double a = valid ? src.value(rowc, f, src.raw(rowc, f)) : 0.0;
                    z = mfma_f64(a, mat[(16 * s + li) * PD + f], z);
                    if (s == nt - 1) dot = fma(a, mu[f], dot);
                }
            }
            double* buf = zs + (s & 1) * (kBlock * kZLd);
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[(16 * wv + lg + 4 * r) * kZLd + li] = z[r];
            __syncthreads();           // (buffer s & 1 is written again at s + 2, behind the barrier of s + 1)
            if (head) {
#pragma unroll
                for (int k = 0; k < kTriPerThread; ++k)
                    for (int c = 0; c < 16; ++c) kd[k] = dd_add(kd[k], dd_two_prod(buf[ki[k] * kZLd + c], buf[kj[k] * kZLd + c]));
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
        // the largest diagonal entry of the binary64 K (its diagonal tiles are numbers 0, 2, 5, 9): above the threshold the
        // slices run again in double-double; below it nothing of the block's arithmetic has changed
        bool large = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int t = wv + 4 * k;
            if (t == 0 || t == 2 || t == 5 || t == 9) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (lg + 4 * r == li) large = large || kacc[k][r] + 1.0 > kDdThreshold;
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
                }
            }
        }
    }
    dot = sum_groups(dot);
    if (lg == 0) {
        const double y = valid ? (double)src.raw_target(rowc) : 0.0;
        sy[16 * wv + li] = y;
        se[16 * wv + li] = valid ? y - dot : 0.0;
    }
    __syncthreads();
    if (head)
        dd_cholesky_packed(km, km + kTriLen);
    else
        gmmvb::blocked_cholesky<kBlock / 16>(km, kKLd, kBlock / 16, dinv);
    if (wv != 0) return;
    auto factor = [&](int i, int j) { return head ? km[tri_at(i, j)] : km[i * kKLd + j]; };      // R_ij, j <= i
    // v = R^-1 e, lane = row
    double acc = se[lane], v = 0.0;
    for (int j = 0; j < kBlock; ++j) {
        const double vj = __shfl(acc, j) / factor(j, j);
        if (lane == j) v = vj;
        if (lane > j) acc = fma(-factor(lane, j), vj, acc);
    }
    const double v2 = v * v;
    sv2[lane] = v2;
    __builtin_amdgcn_wave_barrier();
    double before = 0.0;           // sum of v_j^2 over the block's earlier rows, in row order
    for (int j = 0; j < kBlock - 1; ++j)
        if (j < lane) before += sv2[j];
    const int64_t i = lo + lane;
    if (i >= hi) return;
    const double alpha0 = start[(int64_t)D * D + D + 1];
    const double beta_c = mu[PD], rows_before = mu[PD + 1];
    const double alpha = alpha0 + (rows_before + (double)lane) / 2.0;
    const double beta = beta_c + before / 2.0;
    const double rii = factor(lane, lane);
    const double p_lambda = alpha / (beta * (rii * rii));
    if (out.p_m) out.p_m[i] = sy[lane] - rii * v;
    if (out.p_lambda) out.p_lambda[i] = p_lambda;
    if (out.p_nu) out.p_nu[i] = 2.0 * alpha;
    if (out.nats)
        out.nats[i] = lgamma_half_step(alpha) + 0.5 * log(6.283185307179586477 * alpha / p_lambda)
                      + (alpha + 0.5) * log1p(v2 / (2.0 * beta));
}

}  // namespace regseq
