// Kernels of include/expseq.h: the prequential pass of the scalar conjugate families.  For position i the posterior before
// x[i] is the start posterior plus the statistics S_i of x[0..i-1], so the pass is an exclusive prefix scan of the
// family's statistics followed by a closed form per position.
//
// (1) aggregate_kernel<T, F>: a workgroup (kThreads = 256) owns the tile of kTile = 2048 consecutive positions, a thread
//     kItems = 8 consecutive ones; the tile's statistics go to agg[tile].
// (2) scan_kernel<S>: ONE workgroup of kScanThreads threads.  Thread j folds the aggregates of its ceil(tiles / 256)
//     consecutive tiles, the threads' totals are scanned, and the thread walks its tiles again writing carry[tile], the
//     statistics of everything before the tile.  The count of out-of-domain values goes to the status slot.
// (3) emit_kernel<T, F>: re-reads the tile, scans it from carry[tile], evaluates the closed forms and writes every
//     requested output through LDS, so that a wave stores 512 consecutive bytes.
//
// One fixed tree, shared by (1), (2) and (3) (block_scan): a thread folds its items left to right; a wave scans its 64
// thread totals by Hillis-Steele steps 1, 2, .. 32 (earlier operand on the left); the four wave totals are folded in wave
// order; a thread's base is (carry + waves before) + lanes before, and its items are folded onto the base left to right.
// No floating-point atomics, no waiting between workgroups: the result depends on n alone, never on scheduling.  The operators are integer
// addition, binary64 addition, and for the normal family the (n, mean, m2) merge of include/expfam.h on values shifted by
// the pivot x[0].  tests/expfam_seq_oracle.py restates the tree in NumPy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// No fused multiply-adds in this translation unit: the merge and the closed forms round every operation on its own, so
// that the NumPy restatement of the tree gives the device's bits.
#pragma STDC FP_CONTRACT OFF

namespace expseq {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;
constexpr int kTile = kThreads * kItems;       // EXPSEQ_TILE
constexpr int kScanThreads = 256;              // EXPSEQ_SCAN_THREADS (== kThreads: block_scan serves both)
constexpr int kSlots = 4;                      // 8-byte slots of a tile's aggregate and of its carry
constexpr int kMaxOut = 4;
constexpr int kStage = kTile + kTile / kItems; // staging doubles: item j lives at j + j / 8 (two-way bank conflicts at most)

// (out of line: the library routine's registers would otherwise set the kernel's occupancy)
__device__ __attribute__((noinline)) double lgamma_call(double x) { return lgamma(x); }
// Stirling's tail: lnGamma(x) = (x - 1/2) ln x - x + ln(2 pi) / 2 + t(x); below 1e-19 of truncation error from x = 64 on
// (as in regseq_kernels.h)
__device__ __forceinline__ double stirling_tail(double x) {
    const double r = 1.0 / x, r2 = r * r;
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))));
}
// lnGamma(a) - lnGamma(a + 1/2): from a = 64 on the difference of the two series (regseq_kernels.h: lgamma_half_step)
__device__ __attribute__((noinline)) double lgamma_half_step(double a) {
    if (a < 64.0) return lgamma(a) - lgamma(a + 0.5);
    return -(a * log1p(0.5 / a) + 0.5 * log(a) - 0.5 + (stirling_tail(a + 0.5) - stirling_tail(a)));
}
// lnGamma(r + x) - lnGamma(r), x >= 0: the same difference at step x,
//   (r - 1/2) log1p(x / r) + x ln(r + x) - x + t(r + x) - t(r)
__device__ __attribute__((noinline)) double lgamma_step(double r, double x) {
    if (r < 64.0) return lgamma(r + x) - lgamma(r);
    return (r - 0.5) * log1p(x / r) + x * log(r + x) - x + (stirling_tail(r + x) - stirling_tail(r));
}

__device__ inline double as_double(int64_t v) { return __longlong_as_double((long long)v); }
__device__ inline int64_t as_slot(double v) { return (int64_t)__double_as_longlong(v); }
__device__ inline int64_t shfl_up_i64(int64_t v, int off) { return (int64_t)__shfl_up((long long)v, off); }

struct Out {
    double* p[kMaxOut];      // null = not computed
};
struct Start {
    double v[4];
};

// ---- statistics: identity(), combine(earlier, later), shfl_up, store / load (kSlots slots), bad() ----------------------------
struct Counts {          // bernoulli: ones, zeros
    int64_t c1, c0, nbad;
    static __device__ Counts identity() { return {0, 0, 0}; }
    static __device__ Counts combine(const Counts& a, const Counts& b) { return {a.c1 + b.c1, a.c0 + b.c0, a.nbad + b.nbad}; }
    __device__ Counts shfl_up(int off) const { return {shfl_up_i64(c1, off), shfl_up_i64(c0, off), shfl_up_i64(nbad, off)}; }
    __device__ void store(int64_t* s) const { s[0] = c1, s[1] = c0, s[2] = nbad; }
    static __device__ Counts load(const int64_t* s) { return {s[0], s[1], s[2]}; }
    __device__ int64_t bad() const { return nbad; }
};
struct IntSum {          // poisson
    int64_t sum, nbad;
    static __device__ IntSum identity() { return {0, 0}; }
    static __device__ IntSum combine(const IntSum& a, const IntSum& b) { return {a.sum + b.sum, a.nbad + b.nbad}; }
    __device__ IntSum shfl_up(int off) const { return {shfl_up_i64(sum, off), shfl_up_i64(nbad, off)}; }
    __device__ void store(int64_t* s) const { s[0] = sum, s[1] = nbad; }
    static __device__ IntSum load(const int64_t* s) { return {s[0], s[1]}; }
    __device__ int64_t bad() const { return nbad; }
};
struct FloatSum {        // exponential
    double sum;
    int64_t nbad;
    static __device__ FloatSum identity() { return {0.0, 0}; }
    static __device__ FloatSum combine(const FloatSum& a, const FloatSum& b) { return {a.sum + b.sum, a.nbad + b.nbad}; }
    __device__ FloatSum shfl_up(int off) const { return {__shfl_up(sum, off), shfl_up_i64(nbad, off)}; }
    __device__ void store(int64_t* s) const { s[0] = as_slot(sum), s[1] = nbad; }
    static __device__ FloatSum load(const int64_t* s) { return {as_double(s[0]), s[1]}; }
    __device__ int64_t bad() const { return nbad; }
};
struct Moments {         // normal: of the values minus the pivot
    double n, mean, m2;
    static __device__ Moments identity() { return {0.0, 0.0, 0.0}; }
    static __device__ Moments combine(const Moments& a, const Moments& b) {
        if (b.n == 0.0) return a;
        if (a.n == 0.0) return b;
        const double n = a.n + b.n, d = b.mean - a.mean, r = b.n / n;
        return {n, a.mean + d * r, a.m2 + b.m2 + d * d * a.n * r};
    }
    __device__ Moments shfl_up(int off) const { return {__shfl_up(n, off), __shfl_up(mean, off), __shfl_up(m2, off)}; }
    __device__ void store(int64_t* s) const { s[0] = as_slot(n), s[1] = as_slot(mean), s[2] = as_slot(m2); }
    static __device__ Moments load(const int64_t* s) { return {as_double(s[0]), as_double(s[1]), as_double(s[2])}; }
    __device__ int64_t bad() const { return 0; }
};

// ---- families: item(x) = the statistics of one value; emit = the closed forms at one position ----------------------------------
// emit(i, S, x, start, pivot, want_nats, v): S = statistics of x[0..i-1]; v[0..kParams-1] the parameters, v[kParams] the nats.
template <typename T>
struct Bernoulli {
    using S = Counts;
    static constexpr int kParams = 1;        // p_theta
    static __device__ S item(T x, double) { return {x == (T)1, x == (T)0, (x != (T)0) & (x != (T)1)}; }
    static __device__ void emit(int64_t, const S& s, T x, const Start& st, double, bool nats, double* v) {
        const double a = st.v[0] + (double)s.c1, b = st.v[1] + (double)s.c0, sum = a + b;
        v[0] = a / sum;
        if (nats) v[1] = x == (T)1 ? -log(a / sum) : x == (T)0 ? -log(b / sum) : __builtin_nan("");
    }
};
template <typename T>
struct Poisson {
    using S = IntSum;
    static constexpr int kParams = 2;        // p_r, p_theta
    static __device__ S item(T x, double) { return x < (T)0 ? S{0, 1} : S{(int64_t)x, 0}; }
    static __device__ void emit(int64_t i, const S& s, T x, const Start& st, double, bool nats, double* v) {
        const double r = st.v[0] + (double)s.sum, beta = st.v[1] + (double)i;
        v[0] = r;
        v[1] = 1.0 / (1.0 + beta);
        if (nats) {
            const double xd = (double)x;
            v[2] = x < (T)0 ? __builtin_nan("")
                            : -(lgamma_step(r, xd) - lgamma_call(xd + 1.0) - r * log1p(1.0 / beta) - xd * log1p(beta));
        }
    }
};
template <typename T>
struct Exponential {
    using S = FloatSum;
    static constexpr int kParams = 2;        // p_kappa, p_lambda
    static __device__ S item(T x, double) { return x > (T)0 ? S{(double)x, 0} : S{0.0, 1}; }
    static __device__ void emit(int64_t i, const S& s, T x, const Start& st, double, bool nats, double* v) {
        const double kappa = st.v[0] + (double)i, lambda = st.v[1] + s.sum;
        v[0] = kappa;
        v[1] = lambda;
        if (nats) {
            const double xd = (double)x;
            v[2] = x > (T)0 ? -(log(kappa) - log(lambda + xd) - kappa * log1p(xd / lambda)) : __builtin_nan("");
        }
    }
};
template <typename T>
struct Normal {
    using S = Moments;
    static constexpr int kParams = 3;        // p_mu, p_nu, p_lambda
    static __device__ S item(T x, double pivot) { return {1.0, (double)x - pivot, 0.0}; }
    // normal._fold of (i, pivot + mean, m2) onto (m, kappa, alpha, beta), with every mean held relative to the pivot:
    // the differences it takes are then of the size of the spread, whatever the size of the data
    static __device__ void emit(int64_t, const S& s, T x, const Start& st, double pivot, bool nats, double* v) {
        const double m0 = st.v[0], k0 = st.v[1], n = s.n;
        const double mrel = m0 - pivot, kn = k0 + n, d = s.mean - mrel;
        const double beta = st.v[3] + (s.m2 + n * k0 / kn * (d * d)) / 2.0;
        const double alpha = st.v[2] + n * 0.5;
        const double mu = n == 0.0 ? m0 : pivot + (k0 * mrel + n * s.mean) / kn;
        const double nu = 2.0 * alpha, lambda = kn / (kn + 1.0) * alpha / beta;
        v[0] = mu, v[1] = nu, v[2] = lambda;
        if (nats) {
            const double e = (double)x - mu;
            v[3] = lgamma_half_step(alpha) + 0.5 * log(3.141592653589793238 * nu / lambda)
                   + (nu + 1.0) / 2.0 * log1p(lambda * (e * e) / nu);
        }
    }
};

// The fixed tree over the kThreads totals `t` of a workgroup: returns what lies before the thread inside the workgroup and
// the workgroup's total.  `wave_tot` is kWaves * kSlots slots of LDS; the caller owns the barrier before its reuse.
template <typename S>
__device__ inline S block_scan(const S& t, int64_t* wave_tot, S& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    S inc = t;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const S o = inc.shfl_up(off);
        if (lane >= off) inc = S::combine(o, inc);
    }
    S exc = inc.shfl_up(1);
    if (lane == 0) exc = S::identity();
    if (lane == 63) inc.store(wave_tot + wave * kSlots);
    __syncthreads();
    S base = S::identity(), tot = S::identity();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w == wave) base = tot;
        tot = S::combine(tot, S::load(wave_tot + w * kSlots));
    }
    total = tot;
    return S::combine(base, exc);
}

template <typename T>
__device__ inline void load_items(const T* __restrict__ x, int64_t n, int64_t first, T (&v)[kItems], bool (&in)[kItems]) {
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        in[k] = first + k < n;
        v[k] = in[k] ? x[first + k] : (T)0;
    }
}

template <typename T, typename F>
__device__ inline typename F::S fold_items(const T (&v)[kItems], const bool (&in)[kItems], double pivot) {
    using S = typename F::S;
    S t = S::identity();
#pragma unroll
    for (int k = 0; k < kItems; ++k)
        if (in[k]) t = S::combine(t, F::item(v[k], pivot));
    return t;
}

template <typename T, typename F>
__global__ __launch_bounds__(kThreads) void aggregate_kernel(const T* __restrict__ x, int64_t n, int64_t* __restrict__ agg) {
    using S = typename F::S;
    __shared__ int64_t wave_tot[kWaves * kSlots];
    const double pivot = (double)x[0];
    T v[kItems];
    bool in[kItems];
    load_items(x, n, (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems, v, in);
    S total;
    block_scan(fold_items<T, F>(v, in, pivot), wave_tot, total);
    if (threadIdx.x == 0) total.store(agg + (int64_t)blockIdx.x * kSlots);
}

template <typename S>
__global__ __launch_bounds__(kScanThreads) void scan_kernel(const int64_t* __restrict__ agg, int64_t tiles,
                                                            int64_t* __restrict__ carry, int64_t* __restrict__ status) {
    __shared__ int64_t wave_tot[kWaves * kSlots];
    const int64_t per = (tiles + kScanThreads - 1) / kScanThreads;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < tiles ? lo + per : tiles;
    S t = S::identity();
    for (int64_t k = lo; k < hi; ++k) t = S::combine(t, S::load(agg + k * kSlots));
    S total;
    S run = block_scan(t, wave_tot, total);
    for (int64_t k = lo; k < hi; ++k) {
        run.store(carry + k * kSlots);
        run = S::combine(run, S::load(agg + k * kSlots));
    }
    if (threadIdx.x == 0) status[0] = total.bad();
}

template <typename T, typename F>
__global__ __launch_bounds__(kThreads) void emit_kernel(const T* __restrict__ x, int64_t n, const int64_t* __restrict__ carry,
                                                        Start start, Out out, double* __restrict__ nats) {
    using S = typename F::S;
    constexpr int P = F::kParams;
    __shared__ int64_t wave_tot[kWaves * kSlots];
    __shared__ double stage[kStage];
    const double pivot = (double)x[0];
    const int64_t tile0 = (int64_t)blockIdx.x * kTile, first = tile0 + (int64_t)threadIdx.x * kItems;
    T v[kItems];
    bool in[kItems];
    load_items(x, n, first, v, in);
    S total;
    const S before = block_scan(fold_items<T, F>(v, in, pivot), wave_tot, total);
    S run = S::combine(S::load(carry + (int64_t)blockIdx.x * kSlots), before);
    double val[P + 1][kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        double e[P + 1] = {};
        if (in[k]) {
            F::emit(first + k, run, v[k], start, pivot, nats != nullptr, e);
            run = S::combine(run, F::item(v[k], pivot));
        }
#pragma unroll
        for (int o = 0; o <= P; ++o) val[o][k] = e[o];
    }
    // each requested array in turn: the thread's 8 consecutive entries to LDS, then the tile's entries in position order
#pragma unroll
    for (int o = 0; o <= P; ++o) {
        double* dst = o < P ? out.p[o] : nats;
        if (dst == nullptr) continue;          // (uniform over the grid)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int j = threadIdx.x * kItems + k;
            stage[j + j / kItems] = val[o][k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int j = k * kThreads + threadIdx.x;
            if (tile0 + j < n) dst[tile0 + j] = stage[j + j / kItems];
        }
    }
}

// ---- categorical ------------------------------------------------------------------------------------------------------------
// The statistic is the count of every category, so a position's code length needs one number only: how often its own
// symbol occurred before it.  (1) cat_hist_kernel: a tile's histogram (LDS integer atomics: exact and order-free).
// (2) cat_scan_kernel: one workgroup per category turns the column hist[.][c] into its exclusive prefix over the tiles,
// from the carried count, and carries the total on.  (3) cat_emit_kernel: a workgroup walks its tile 256 positions at a time
// with the running counts in LDS; inside a wave the lanes with the same symbol find each other by ballots over the
// symbol's bits, a lane's rank among them is a popcount, and the waves of a step take their turns in order.
// (4) cat_rows_kernel, only when rows or the argmax are asked for: one wave per tile walks the positions in order with the
// whole count vector in LDS, its lanes striding over the categories.
// The one-hot form first reduces every row to its index (onehot_index_kernel), -1 for a row expfam.h calls bad.

template <typename T>
__device__ inline bool cat_valid(T v, int degree) {
    return (int64_t)v >= 0 && (int64_t)v < (int64_t)degree;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void onehot_index_kernel(const T* __restrict__ x, int64_t m, int degree, int64_t ld,
                                                                int64_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= m) return;          // (a whole wave; the kernel has no barrier)
    const T* r = x + row * ld;
    long long sum = 0;
    int neg = 0, at = -1;
    for (int c = lane; c < degree; c += 64) {
        const T v = r[c];
        sum += (long long)v;
        neg |= (long long)v < 0;
        if (v != (T)0) at = c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        neg |= __shfl_xor(neg, off);
        const int o = __shfl_xor(at, off);
        at = o > at ? o : at;
    }
    if (lane == 0) idx[row] = (neg || sum != 1) ? -1 : at;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cat_hist_kernel(const T* __restrict__ x, int64_t m, int degree,
                                                            int64_t* __restrict__ hist, int64_t* __restrict__ bad) {
    extern __shared__ unsigned bins[];          // degree, then the tile's bad count
    for (int c = threadIdx.x; c <= degree; c += kThreads) bins[c] = 0u;
    __syncthreads();
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int64_t i = tile0 + k * kThreads + threadIdx.x;
        if (i < m) {
            const T v = x[i];
            atomicAdd(&bins[cat_valid(v, degree) ? (int)v : degree], 1u);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < degree; c += kThreads) hist[(int64_t)blockIdx.x * degree + c] = (int64_t)bins[c];
    if (threadIdx.x == 0) bad[blockIdx.x] = (int64_t)bins[degree];
}

// Workgroup c < degree scans the column hist[.][c] over the tiles (thread j its ceil(tiles / 256) consecutive tiles, the
// threads' totals through block_scan: integers, so the order is free); workgroup `degree` adds up the tiles' bad counts.
__global__ __launch_bounds__(kThreads) void cat_scan_kernel(int64_t* __restrict__ hist, const int64_t* __restrict__ bad,
                                                            int64_t tiles, int degree, int64_t* __restrict__ counts,
                                                            int64_t* __restrict__ status, int first_chunk) {
    __shared__ int64_t wave_tot[kWaves * kSlots];
    const int c = blockIdx.x;
    const bool column = c < degree;
    const int64_t per = (tiles + kThreads - 1) / kThreads;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < tiles ? lo + per : tiles;
    const int64_t carried = column ? counts[c] : (first_chunk ? 0 : status[0]);          // (read before block_scan's barrier)
    IntSum t = IntSum::identity();
    for (int64_t k = lo; k < hi; ++k) t.sum += column ? hist[k * degree + c] : bad[k];
    IntSum total;
    const IntSum before = block_scan(t, wave_tot, total);
    if (column) {
        int64_t run = carried + before.sum;
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t h = hist[k * degree + c];
            hist[k * degree + c] = run;
            run += h;
        }
    }
    if (threadIdx.x == 0) (column ? counts[c] : status[0]) = carried + total.sum;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cat_emit_kernel(const T* __restrict__ x, int64_t m, int degree,
                                                            const int64_t* __restrict__ offs, const double* __restrict__ alpha,
                                                            double s0, int64_t i0, double* __restrict__ nats) {
    extern __shared__ long long cur[];          // degree: occurrences before the position the walk has reached
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < degree; c += kThreads) cur[c] = offs[(int64_t)blockIdx.x * degree + c];
    __syncthreads();
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    for (int step = 0; step < kItems; ++step) {
        const int64_t i = tile0 + step * kThreads + threadIdx.x;
        const bool in = i < m;
        const T v = in ? x[i] : (T)0;
        const bool valid = in && cat_valid(v, degree);
        const int k = valid ? (int)v : 0;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; (1 << b) < degree; ++b) {
            const bool bit = (k >> b) & 1;
            const unsigned long long has = __ballot(bit);
            peers &= bit ? has : ~has;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        const bool last = valid && (peers >> lane) == 1ull;
        long long before = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) {
                if (valid) before = cur[k];
                __builtin_amdgcn_wave_barrier();
                if (last) cur[k] = before + __popcll(peers);
            }
            __syncthreads();
        }
        if (in) nats[i] = valid ? -log((alpha[k] + (double)(before + rank)) / (s0 + (double)(i0 + i))) : __builtin_nan("");
    }
}

template <typename T>
__global__ __launch_bounds__(64) void cat_rows_kernel(const T* __restrict__ x, int64_t m, int degree,
                                                      const int64_t* __restrict__ offs, const double* __restrict__ alpha,
                                                      double s0, int64_t i0, double* __restrict__ rows,
                                                      int64_t* __restrict__ argmax) {
    extern __shared__ long long cur[];          // degree counts, then degree binary64 alpha
    double* a = (double*)(cur + degree);
    const int lane = threadIdx.x;
    for (int c = lane; c < degree; c += 64) {
        cur[c] = offs[(int64_t)blockIdx.x * degree + c];
        a[c] = alpha[c];
    }
    __syncthreads();
    const int64_t tile0 = (int64_t)blockIdx.x * kTile, end = tile0 + kTile < m ? tile0 + kTile : m;
    for (int64_t i = tile0; i < end; ++i) {
        const double norm = s0 + (double)(i0 + i);
        double best = -1.0;
        int at = 0x7fffffff;
        for (int c = lane; c < degree; c += 64) {
            const double q = (a[c] + (double)cur[c]) / norm;
            if (rows) rows[i * degree + c] = q;
            if (q > best) best = q, at = c;          // (ascending c: the lane's first maximum)
        }
        if (argmax) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off);
                const int oa = __shfl_xor(at, off);
                if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
            }
            if (lane == 0) argmax[i] = at;
        }
        const T v = x[i];
        if (cat_valid(v, degree) && lane == ((int)v & 63)) cur[(int)v] += 1;
        __syncthreads();          // (one wave: orders the LDS update before the next position's reads)
    }
}

}  // namespace expseq
