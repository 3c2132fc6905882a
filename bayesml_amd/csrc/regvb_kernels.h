// Kernels of the Normal-Gamma regression family (include/regvb.h): linearregression and autoregressive.
//
// (a) gram_kernel: one pass over the rows w_n (and targets y_n) accumulates, in f64,
//       G = sum_n w_n w_n^T  (upper tile pairs on v_mfma_f64_16x16x4_f64),  c = sum_n w_n y_n,  s = sum_n y_n^2,  n.
//     Replaces x.T @ x, x.T @ y, y @ y of bayesml/linearregression/_linearregression.py:544-548 and, fed by the lag-window
//     row source, the Python loop over T that builds x_mat in bayesml/autoregressive/_autoregressive.py:481-503.
//     The sample index is the MFMA contraction index and the tile ownership is the wide M-step's (mstep.h, mstep_wide_body):
//     with T (even) feature tiles the workgroup has T / 2 waves, wave w owns the A-operand tiles w and T - 1 - w, i.e. the tile
//     pairs (t2, w), t2 >= w, and (t2, T - 1 - w), t2 >= T - 1 - w: T + 1 accumulator tiles each.  The workgroup stages a batch
//     of 16 rows - widened to f64, zero padded to 16 T features - into LDS in the order the operands are read (element (row r,
//     feature f) at ((r >> 2) T + (f >> 4)) 64 + (r & 3) 16 + (f & 15), so the operand of (step, tile) is the lane-linear read
//     sx[(st T + t) 64 + lane]), a batch ahead through registers, two buffers, one barrier per batch.  No responsibilities, no
//     pivot, nothing N-sized besides the caller's rows.  Every workgroup owns a contiguous row range and writes one slab;
//     gram_reduce_kernel adds the slabs in split order: no atomics, two runs give the same bits, and the statistics of two
//     row ranges add.
// (b) WindowRows: the row source of (a) for a series x[0 .. len): row n is [1, x[t - p], ..., x[t - 1]] with target x[t],
//     t = n + t0 (t0 = p without padding, 0 with zeros at negative times).  The [len, p + 1] matrix is never made: the rows
//     exist only in the LDS batch of (a).
// (c) predict_kernel: per row  m = x . mu  and  q = |L^-1 x|^2  (Lambda = L L^T), written as p_ms = m and
//     p_lambdas = scale / (1 + q) (bayesml/linearregression/_linearregression.py:717-718, which solves a D x N system).
//     z = L^-1 x on f64 MFMA: output tile (16 entries of z) x (16 rows), contraction over the features; the factor comes
//     through LDS by block columns, packed beforehand in operand order (pack_factor_kernel) so that staging is a straight
//     copy; the zero tiles right of the diagonal are skipped (D^2 flop per row executed instead of 2 D^2).
#pragma once
#include <utility>
#include "common.h"

namespace regvb {
using gmmvb::d4;
using gmmvb::mfma_f64;
using gmmvb::pair_index;
using gmmvb::sum_groups;
using gmmvb::tri_pairs;

constexpr int kBatch = 16;          // rows per LDS batch of the Gram kernel
// Row ranges (workgroups, slabs) of one Gram launch: about what 256 CUs hold at once.  Up to T = 8 a wave takes 126 to
// 166 registers (VGPRs + AGPRs; three waves per SIMD, twelve per CU, T / 2 per workgroup): 768 workgroups at T = 8, 1024 at
// T = 6, and no more than 1536 below (more slabs only lengthen the reduce).  From T = 10 on a wave takes 188 to 246 and a
// CU holds one workgroup: 256.  The scratch is gram_max_splits(T) slabs: 10, 32, 45, 57, 29, 41, 55, 71 MB for T = 2 .. 16.
__host__ __device__ constexpr int gram_max_splits(int t) {
    return t > 8 ? 256 : (256 * (12 / (t / 2)) < 1536 ? 256 * (12 / (t / 2)) : 1536);
}
// Waves per workgroup of the predictive kernel, 16 rows each.  Eight share one copy of the factor in LDS; above ten tiles
// the T accumulator tiles want the AGPRs, which a 512-thread workgroup (256 registers per wave) does not leave: four.
__host__ __device__ constexpr int predict_waves(int t) { return t > 10 ? 4 : 8; }

// Slab of one row range:  [ P tile pairs x (4 regs x 64 lanes) | c[16 T] | s | n | pad ]
__host__ __device__ constexpr int64_t gram_slab_len(int t) { return (int64_t)tri_pairs(t) * 256 + 16 * t + 16; }
// even number of 16-feature tiles that holds D features
__host__ __device__ constexpr int even_tiles(int D) { return 2 * ((D + 31) / 32); }

// ---- row sources ---------------------------------------------------------------------------------------------------------
// raw(n, f) / raw_target(n) are plain loads in the storage dtype from an address that is always valid (feature and time
// indices clamped), so that nothing has to wait for them where they are issued; value(n, f, raw) is what the element is.
// (x and y have dtypes of their own: f32 regressors with f64 targets are read as they are, nothing is narrowed)
template <typename XT, typename YT>
struct MatrixRows {
    typedef XT raw_t;
    typedef YT target_t;
    const XT* x;
    int64_t ldx;
    const YT* y;
    int D;
    __device__ __forceinline__ XT raw(int64_t n, int f) const { return x[n * ldx + (f < D ? f : D - 1)]; }
    __device__ __forceinline__ double value(int64_t, int f, XT v) const { return f < D ? (double)v : 0.0; }
    __device__ __forceinline__ YT raw_target(int64_t n) const { return y[n]; }
};
template <typename XT>
struct WindowRows {
    typedef XT raw_t;
    typedef XT target_t;
    const XT* x;      // the series
    int p;            // degree: D = p + 1 features
    int64_t t0;       // time of row 0
    // feature f >= 1 of row n is x[n + t0 - p + f - 1] (oldest first), zero at negative times
    __device__ __forceinline__ int64_t time(int64_t n, int f) const { return n + t0 - p + (f < 1 ? 1 : (f > p ? p : f)) - 1; }
    __device__ __forceinline__ XT raw(int64_t n, int f) const {
        const int64_t s = time(n, f);
        return x[s > 0 ? s : 0];       // (p = 0: time() = n + t0 - 1 may be -1 for the constant column)
    }
    __device__ __forceinline__ double value(int64_t n, int f, XT v) const {
        if (f == 0) return 1.0;
        return (f <= p && time(n, f) >= 0) ? (double)v : 0.0;
    }
    __device__ __forceinline__ XT raw_target(int64_t n) const { return x[n + t0]; }
};

// ---- (a) -----------------------------------------------------------------------------------------------------------------
template <int T, int SUB, typename SRC>
__device__ __forceinline__ void gram_body(const SRC& src, int64_t lo, int64_t hi, double* __restrict__ out,
                                          double* __restrict__ sx, double* __restrict__ sy) {
    static_assert(T >= 2 && T <= 16 && T % 2 == 0, "even tile counts");
    constexpr int P = tri_pairs(T);
    constexpr int C1 = SUB, C2 = T - 1 - SUB;      // the wave's A-operand tiles (C1 < C2)
    constexpr int N1 = T - C1, N2 = T - C2;
    constexpr int BUF = kBatch * 16 * T;
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    d4 acc1[N1], acc2[N2];
#pragma unroll
    for (int p = 0; p < N1; ++p) acc1[p] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int p = 0; p < N2; ++p) acc2[p] = d4{0.0, 0.0, 0.0, 0.0};
    double c1 = 0.0, c2 = 0.0, ss = 0.0;
    // staging: 32 T threads, 16 x 16 T elements: thread -> feature f, rows rsel, rsel + 2, ... (rows past hi are zero)
    const int f = tid % (16 * T), rsel = tid / (16 * T);
    const int sidx = (f >> 4) * 64 + (f & 15);
    // The loads of request() are consumed by deposit(), a batch of MFMAs later: raw values from clamped (always valid)
    // addresses, no conversion and no range test in between, so that no s_waitcnt lands in front of the MFMAs.
    typename SRC::raw_t v[8];
    typename SRC::target_t yv = 0;
    auto request = [&](int64_t row0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t row = row0 + 2 * k + rsel;
            v[k] = src.raw(row < hi ? row : hi - 1, f);
        }
        if (tid < kBatch) yv = src.raw_target(row0 + tid < hi ? row0 + tid : hi - 1);
    };
    auto deposit = [&](int64_t row0, double* dx, double* dy) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = 2 * k + rsel;
            dx[(r >> 2) * T * 64 + (r & 3) * 16 + sidx] = row0 + r < hi ? src.value(row0 + r, f, v[k]) : 0.0;
        }
        if (tid < kBatch) dy[tid] = row0 + tid < hi ? (double)yv : 0.0;
    };
    request(lo);
    deposit(lo, sx, sy);
    __syncthreads();
    int b = 0;
    for (int64_t r0 = lo; r0 < hi; r0 += kBatch, b ^= 1) {
        const bool more = r0 + kBatch < hi;        // (workgroup uniform)
        if (more) request(r0 + kBatch);            // in flight while this batch is worked through
        __builtin_amdgcn_sched_barrier(0);
        const double* cur = sx + b * BUF;
        const double* cy = sy + b * kBatch;
#pragma unroll
        for (int st = 0; st < kBatch / 4; ++st) {
            const double yq = cy[4 * st + g];
            double xv[N1];                         // tiles C1 .. T - 1 of the step's four rows
#pragma unroll
            for (int p = 0; p < N1; ++p) xv[p] = cur[(st * T + C1 + p) * 64 + lane];
            const double a1 = xv[0], a2 = xv[C2 - C1];
            c1 = fma(a1, yq, c1);
            c2 = fma(a2, yq, c2);
            if (SUB == 0) ss = fma(yq, yq, ss);
#pragma unroll
            for (int p = 0; p < N1; ++p) acc1[p] = mfma_f64(a1, xv[p], acc1[p]);
#pragma unroll
            for (int p = 0; p < N2; ++p) acc2[p] = mfma_f64(a2, xv[C2 - C1 + p], acc2[p]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) deposit(r0 + kBatch, sx + (b ^ 1) * BUF, sy + (b ^ 1) * kBatch);
        __syncthreads();                           // the next batch is in LDS; everybody is done with this one
    }
#pragma unroll
    for (int p = 0; p < N1; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(pair_index(C1 + p, C1) * 4 + r) * 64 + lane] = acc1[p][r];
#pragma unroll
    for (int p = 0; p < N2; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(pair_index(C2 + p, C2) * 4 + r) * 64 + lane] = acc2[p][r];
    {
        const double t1 = sum_groups(c1), t2 = sum_groups(c2);
        if (g == 0) {
            out[P * 256 + 16 * C1 + i] = t1;
            out[P * 256 + 16 * C2 + i] = t2;
        }
    }
    if (SUB == 0) {
        const double s = sum_groups(ss);           // (every lane of a group holds the same four rows' share)
        if (lane == 0) {
            out[P * 256 + 16 * T + 0] = s;
            out[P * 256 + 16 * T + 1] = (double)(hi - lo);
        }
    }
}

template <int T, typename SRC, int... I>
__device__ __forceinline__ void gram_dispatch(int sub, const SRC& src, int64_t lo, int64_t hi, double* __restrict__ out,
                                              double* __restrict__ sx, double* __restrict__ sy,
                                              std::integer_sequence<int, I...>) {
    ((sub == I ? gram_body<T, I>(src, lo, hi, out, sx, sy) : (void)0), ...);
}

template <int T, typename SRC>
__global__ __launch_bounds__(32 * T) void gram_kernel(SRC src, int64_t n_rows, int64_t rows_per_split,
                                                      double* __restrict__ slabs /*[S][gram_slab_len(T)]*/) {
    __shared__ __attribute__((aligned(16))) double sx[2 * kBatch * 16 * T];      // 64 KB at T = 16
    __shared__ double sy[2 * kBatch];
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t lo = (int64_t)blockIdx.x * rows_per_split;
    int64_t hi = lo + rows_per_split;
    if (hi > n_rows) hi = n_rows;
    double* out = slabs + (int64_t)blockIdx.x * gram_slab_len(T);
    gram_dispatch<T>(sub, src, lo, hi, out, sx, sy, std::make_integer_sequence<int, T / 2>{});
}

// stats = [ G[D][D] | c[D] | s | n ]: the slabs added in split order, G unpacked to the full symmetric matrix
static __global__ void gram_reduce_kernel(const double* __restrict__ slabs, int S, int T, int D, double* __restrict__ stats) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t len = (int64_t)D * D + D + 2;
    if (e >= len) return;
    const int64_t slab = gram_slab_len(T);
    const int P = tri_pairs(T);
    int64_t idx;
    if (e < (int64_t)D * D) {
        int u = (int)(e / D), w = (int)(e % D);
        if (u > w) {       // one of the two mirror elements is computed: the one above the diagonal
            const int t = u;
            u = w;
            w = t;
        }
        const int t1 = u >> 4, t2 = w >> 4, m = u & 15;
        idx = ((int64_t)pair_index(t2, t1) * 4 + (m >> 2)) * 64 + (m & 3) * 16 + (w & 15);
    } else {
        idx = (int64_t)P * 256 + (e - (int64_t)D * D < D ? e - (int64_t)D * D : 16 * T + (e - (int64_t)D * D - D));
    }
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += slabs[s * slab + idx];
    stats[e] = a;
}

// ---- (c) -----------------------------------------------------------------------------------------------------------------
// The factor is packed by block COLUMNS of 16 features: column c holds the tiles (tj, c), tj = c .. T - 1, each as four
// contraction steps e of 64 lanes: packed[packed_offset(T, c) + ((tj - c) 4 + e) 64 + lane] = Linv[16 tj + i][16 c + 4 g + e]
// (lane = 16 g + i; zero outside the D x D lower triangle).
__host__ __device__ constexpr int64_t packed_offset(int t, int c) { return 256 * ((int64_t)c * t - (int64_t)c * (c - 1) / 2); }
__host__ __device__ constexpr int64_t packed_len(int t) { return packed_offset(t, t); }      // 128 T (T + 1)

static __global__ void pack_factor_kernel(const double* __restrict__ linv /*[D][D] row-major*/, int D, int T,
                                          double* __restrict__ packed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= packed_len(T)) return;
    int c = 0;
    while (packed_offset(T, c + 1) <= e) ++c;
    const int64_t o = e - packed_offset(T, c);
    const int lane = (int)(o & 63), i = lane & 15, g = lane >> 4;
    const int step = (int)(o >> 6), tj = c + (step >> 2);
    const int row = 16 * tj + i, col = 16 * c + 4 * g + (step & 3);
    packed[e] = (row < D && col <= row) ? linv[(int64_t)row * D + col] : 0.0;
}

// A workgroup of predict_waves(T) waves takes 16 rows per wave: lane (i, g) works on row i and, of every 16-feature chunk c,
// on features 16 c + 4 g .. + 3 (the contraction order is free as long as both operands agree).  The wave keeps the T
// output tiles of z = Linv x (16 entries x 16 rows each) in registers and walks the chunks once: chunk c feeds the tiles
// tj >= c (the factor is lower triangular: the tiles right of the diagonal are never executed), its four feature values
// per lane arrive from global memory a chunk ahead, the factor's block column c through LDS a column ahead (two buffers,
// one barrier per chunk).
template <int T, typename XT>
__global__ __launch_bounds__(64 * predict_waves(T)) void predict_kernel(const XT* __restrict__ x, int64_t ldx, int64_t n_rows, int D,
                                                      const double* __restrict__ mu, const double* __restrict__ packed,
                                                      double scale, double* __restrict__ p_ms, double* __restrict__ p_lambdas) {
    constexpr int NT = 64 * predict_waves(T);
    constexpr int BLK = 256 * T;                                   // doubles of the largest block column (c = 0)
    constexpr int KMAX = (BLK + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) double sl[2 * BLK];      // 64 KB at T = 16
    __shared__ double smu[16 * T];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * (16 * predict_waves(T)) + wave * 16 + i;
    const int64_t rowc = row < n_rows ? row : n_rows - 1;
    XT xn[4];
    auto request_x = [&](int c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {          // (address clamped, the range test waits until the value is used)
            const int f = 16 * c + 4 * g + e;
            xn[e] = x[rowc * ldx + (f < D ? f : D - 1)];
        }
    };
    request_x(0);
    for (int f = tid; f < 16 * T; f += NT) smu[f] = f < D ? mu[f] : 0.0;
    for (int e = tid; e < BLK; e += NT) sl[e] = packed[e];         // block column 0
    __syncthreads();
    d4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    double m = 0.0;
#pragma unroll
    for (int c = 0; c < T; ++c) {
        const double* cur = sl + (c & 1) * BLK;
        double* nxt = sl + ((c + 1) & 1) * BLK;
        double xc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xc[e] = 16 * c + 4 * g + e < D ? (double)xn[e] : 0.0;
        double st[KMAX];
        const int nn = 256 * (T - c - 1);                            // doubles of block column c + 1
        if (c + 1 < T) {
            request_x(c + 1);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (NT * k < nn) st[k] = packed[packed_offset(T, c + 1) + (tid + NT * k < nn ? tid + NT * k : 0)];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m = fma(xc[e], smu[16 * c + 4 * g + e], m);
#pragma unroll
            for (int tj = c; tj < T; ++tj) acc[tj] = mfma_f64(cur[((tj - c) * 4 + e) * 64 + lane], xc[e], acc[tj]);
            // (keeps hipcc from hoisting every LDS operand of the chunk above its first MFMA: 64 doubles at T = 16, which
            // spilled the accumulators to scratch)
            __builtin_amdgcn_sched_barrier(0);
        }
        if (c + 1 < T) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (NT * k < nn && tid + NT * k < nn) nxt[tid + NT * k] = st[k];
            __syncthreads();
        }
    }
    double q = 0.0;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) q = fma(acc[t][r], acc[t][r], q);
    m = sum_groups(m);
    q = sum_groups(q);
    if (g == 0 && row < n_rows) {
        p_ms[row] = m;
        p_lambdas[row] = scale / (1.0 + q);
    }
}

}  // namespace regvb
