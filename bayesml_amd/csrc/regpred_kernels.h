// Kernels of include/regpred.h: held-out scoring under a fixed Normal-Gamma posterior, and the lag windows of many series.
//
// (a) The row map.  Row r of a call over n_seq series is position t of series s; nothing n-sized says which.  A workgroup
//     owns a contiguous row range [lo, hi): it bisects the row-offset table roff twice (for lo and for hi - 1), which
//     bounds the series its rows can belong to, and stages that slice of roff and of the value offsets off in LDS
//     (stage_rows; up to kSlice entries, otherwise the slice stays where it is, in L2).  locate(r) is then a bisection of
//     a few LDS entries; a tie in roff is a series without rows, and "the last entry at or below r" steps over it.  A batch
//     of 16 rows may hold the ends and starts of several series: every row is located on its own, so nothing in the
//     kernels knows about batches and boundaries at all.
// (b) SegWindowRows: element (row, lag j) is x[pos - j] when pos - j >= the series' own start, else zero; the address is
//     clamped into the series, as WindowRows does, so that the load is always valid and the range test waits until the
//     value is used.  It is both a source of regvb's gram_body (raw / value / raw_target by row number) and of score_kernel
//     (the same by located row).
// (c) score_kernel: regvb's predict_kernel - z = L^-1 w on v_mfma_f64_16x16x4_f64, rows as the N index, contraction over
//     the features, the packed factor through LDS by block columns, zero tiles right of the diagonal skipped - with a row
//     source instead of a matrix pointer and the Student-t finished in registers: one double per row leaves the kernel.
// (d) seg_gram_kernel: gram_body of regvb_kernels.h over the segmented source; slabs and gram_reduce_kernel are regvb's.
// (e) segment_sum_kernel: a wave per segment, 64 strided partial sums in row order, then a butterfly.
#pragma once
#include "regvb_kernels.h"

namespace regpred {
using gmmvb::d4;
using gmmvb::mfma_f64;
using gmmvb::sum_groups;
using regvb::packed_offset;
using regvb::predict_waves;

constexpr int kSlice = 512;         // table entries a workgroup stages in LDS (2 x 4 KB)
constexpr int kSumWaves = 4;        // waves per workgroup of segment_sum_kernel

// ---- (a) -----------------------------------------------------------------------------------------------------------------
// the largest k in [0, cnt) with tab[k] <= r; tab[0] <= r < tab[cnt]
__device__ __forceinline__ int64_t last_at_or_below(const int64_t* tab, int64_t cnt, int64_t r) {
    int64_t lo = 0, hi = cnt;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tab[mid] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct RowMap {
    const int64_t* roff;      // cnt + 1 row offsets: roff[0] <= every row asked for < roff[cnt]
    const int64_t* off;       // the value offsets of the same cnt series
    int64_t cnt;
};

// The map of the rows [lo, hi) (lo < hi, the same for the whole workgroup; every thread calls it: it holds a barrier).
__device__ __forceinline__ RowMap stage_rows(const int64_t* __restrict__ roff, const int64_t* __restrict__ off, int64_t n_seq,
                                             int64_t lo, int64_t hi, int64_t* s_roff, int64_t* s_off) {
    const int64_t s_lo = last_at_or_below(roff, n_seq, lo), s_hi = last_at_or_below(roff, n_seq, hi - 1);
    const int64_t cnt = s_hi - s_lo + 1;
    const bool fits = cnt + 1 <= kSlice;
    if (fits)
        for (int64_t k = threadIdx.x; k <= cnt; k += blockDim.x) {
            s_roff[k] = roff[s_lo + k];
            if (k < cnt) s_off[k] = off[s_lo + k];
        }
    __syncthreads();
    return fits ? RowMap{s_roff, s_off, cnt} : RowMap{roff + s_lo, off + s_lo, cnt};
}

// ---- (b) -----------------------------------------------------------------------------------------------------------------
template <typename XT>
struct SegWindowRows {
    typedef XT raw_t;
    typedef XT target_t;
    struct At {
        int64_t pos, start;   // the row's target is x[pos]; its series starts at x[start]
    };
    const XT* x;
    int64_t length;           // of the whole array
    int p;                    // degree: D = p + 1 features
    int64_t t0;               // position of a series' first row: p without padding, 0 with zeros before the start
    RowMap map;
    __device__ __forceinline__ At locate(int64_t n) const {
        const int64_t k = last_at_or_below(map.roff, map.cnt, n);
        const int64_t start = map.off[k];
        return At{start + t0 + (n - map.roff[k]), start};
    }
    // feature f >= 1 of a row is x[pos - p + f - 1] (oldest first), zero before the series' start
    __device__ __forceinline__ int64_t time(At a, int f) const { return a.pos - p + (f < 1 ? 1 : (f > p ? p : f)) - 1; }
    __device__ __forceinline__ int64_t clamped(At a, int64_t s) const {
        s = s > a.start ? s : a.start;
        return s < length ? s : length - 1;
    }
    __device__ __forceinline__ XT raw(At a, int f) const { return x[clamped(a, time(a, f))]; }
    __device__ __forceinline__ double value(At a, int f, XT v) const {
        if (f == 0) return 1.0;
        return (f <= p && time(a, f) >= a.start) ? (double)v : 0.0;
    }
    __device__ __forceinline__ XT raw_target(At a) const { return x[clamped(a, a.pos)]; }
    // by row number: what gram_body asks for
    __device__ __forceinline__ XT raw(int64_t n, int f) const { return raw(locate(n), f); }
    __device__ __forceinline__ double value(int64_t n, int f, XT v) const { return value(locate(n), f, v); }
    __device__ __forceinline__ XT raw_target(int64_t n) const { return raw_target(locate(n)); }
};

// What a kernel is handed, and what it opens for its row range.
template <typename XT>
struct SegWindowArgs {
    const XT* x;
    int64_t length;
    int p;
    int64_t t0;
    const int64_t* roff;
    const int64_t* off;
    int64_t n_seq;
    __device__ __forceinline__ SegWindowRows<XT> open(int64_t lo, int64_t hi, int64_t* s_roff, int64_t* s_off) const {
        return SegWindowRows<XT>{x, length, p, t0, stage_rows(roff, off, n_seq, lo, hi, s_roff, s_off)};
    }
};
template <typename XT, typename YT>
struct MatrixArgs : regvb::MatrixRows<XT, YT> {      // a matrix row is located by its number
    __device__ __forceinline__ const MatrixArgs& open(int64_t, int64_t, int64_t*, int64_t*) const { return *this; }
    __device__ __forceinline__ int64_t locate(int64_t n) const { return n; }
};

// ---- (c) -----------------------------------------------------------------------------------------------------------------
struct StudentT {
    double scale, nu, c0;     // alpha / beta, 2 alpha, lnGamma((nu + 1) / 2) - lnGamma(nu / 2) - ln(pi nu) / 2
};

// predict_kernel's walk (regvb_kernels.h): lane (i, g) works on row i of its wave's sixteen and, of every 16-feature chunk
// c, on features 16 c + 4 g .. + 3; chunk c feeds the output tiles tj >= c; the features arrive a chunk ahead, the factor's
// block column a column ahead through LDS (two buffers, one barrier per chunk).  The register budget is predict_kernel's
// (T accumulator tiles; the located row adds four registers), hence its predict_waves(T).
template <int T, typename ARG>
__global__ __launch_bounds__(64 * predict_waves(T)) void score_kernel(ARG arg, int64_t n_rows, int D, const double* __restrict__ mu,
                                                                      const double* __restrict__ packed, StudentT k,
                                                                      double* __restrict__ lnp) {
    constexpr int NT = 64 * predict_waves(T);
    constexpr int ROWS = 16 * predict_waves(T);
    constexpr int BLK = 256 * T;                                   // doubles of the largest block column (c = 0)
    constexpr int KMAX = (BLK + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) double sl[2 * BLK];      // 64 KB at T = 16
    __shared__ double smu[16 * T];
    __shared__ int64_t s_roff[kSlice], s_off[kSlice];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int64_t hi = row0 + ROWS < n_rows ? row0 + ROWS : n_rows;
    const auto src = arg.open(row0, hi, s_roff, s_off);
    const int64_t row = row0 + wave * 16 + i;
    const auto at = src.locate(row < hi ? row : hi - 1);
    decltype(src.raw(at, 0)) xn[4];
    auto request_x = [&](int c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xn[e] = src.raw(at, 16 * c + 4 * g + e);      // (address clamped by the source)
    };
    request_x(0);
    const auto yv = src.raw_target(at);
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
        for (int e = 0; e < 4; ++e) xc[e] = src.value(at, 16 * c + 4 * g + e, xn[e]);
        double st[KMAX];
        const int nn = 256 * (T - c - 1);                            // doubles of block column c + 1
        if (c + 1 < T) {
            request_x(c + 1);
#pragma unroll
            for (int kk = 0; kk < KMAX; ++kk)
                if (NT * kk < nn) st[kk] = packed[packed_offset(T, c + 1) + (tid + NT * kk < nn ? tid + NT * kk : 0)];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m = fma(xc[e], smu[16 * c + 4 * g + e], m);
#pragma unroll
            for (int tj = c; tj < T; ++tj) acc[tj] = mfma_f64(cur[((tj - c) * 4 + e) * 64 + lane], xc[e], acc[tj]);
            __builtin_amdgcn_sched_barrier(0);      // (predict_kernel: keeps the chunk's LDS operands from being hoisted)
        }
        if (c + 1 < T) {
#pragma unroll
            for (int kk = 0; kk < KMAX; ++kk)
                if (NT * kk < nn && tid + NT * kk < nn) nxt[tid + NT * kk] = st[kk];
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
    if (g == 0 && row < hi) {
        const double lam = k.scale / (1.0 + q), d = (double)yv - m;
        lnp[row] = k.c0 + 0.5 * log(lam) - 0.5 * (k.nu + 1.0) * log1p(lam * d * d / k.nu);
    }
}

// ---- (d) -----------------------------------------------------------------------------------------------------------------
// regvb's gram_kernel with the source opened for the workgroup's row range (same ranges, same slabs, same reduce).
template <int T, typename ARG>
__global__ __launch_bounds__(32 * T) void seg_gram_kernel(ARG arg, int64_t n_rows, int64_t rows_per_split,
                                                          double* __restrict__ slabs /*[S][gram_slab_len(T)]*/) {
    __shared__ __attribute__((aligned(16))) double sx[2 * regvb::kBatch * 16 * T];
    __shared__ double sy[2 * regvb::kBatch];
    __shared__ int64_t s_roff[kSlice], s_off[kSlice];
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t lo = (int64_t)blockIdx.x * rows_per_split;
    int64_t hi = lo + rows_per_split;
    if (hi > n_rows) hi = n_rows;
    const auto src = arg.open(lo, hi, s_roff, s_off);
    double* out = slabs + (int64_t)blockIdx.x * regvb::gram_slab_len(T);
    regvb::gram_dispatch<T>(sub, src, lo, hi, out, sx, sy, std::make_integer_sequence<int, T / 2>{});
}

// ---- (e) -----------------------------------------------------------------------------------------------------------------
// out[s] = sum of v[lo_s .. hi_s): the segments are tab[s] .. tab[s + 1], or, without a table, the chunks of `chunk`
// entries of v[0 .. n).  Lane l adds the entries l, l + 64, ... in order, then the butterfly: the shape depends on the
// segment's length alone.
static __global__ __launch_bounds__(64 * kSumWaves) void segment_sum_kernel(const int64_t* __restrict__ tab, int64_t chunk,
                                                                            int64_t n, int64_t n_seg,
                                                                            const double* __restrict__ v,
                                                                            double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kSumWaves + (threadIdx.x >> 6);
    if (s >= n_seg) return;
    const int64_t lo = tab ? tab[s] : s * chunk;
    int64_t hi = tab ? tab[s + 1] : lo + chunk;
    if (!tab && hi > n) hi = n;
    double acc = 0.0;
    for (int64_t t = lo + lane; t < hi; t += 64) acc += v[t];
    acc = gmmvb::sum_wave(acc);
    if (lane == 0) out[s] = acc;
}

}  // namespace regpred
