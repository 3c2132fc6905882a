// Kernels of include/expfam.h: one streaming validate-and-reduce pass per scalar conjugate family.
//
// (a) stream_kernel<T, ACC>: every workgroup (256 threads) owns a contiguous range of 16-byte vectors of the sample, which
//     starts at the first 16-byte boundary at or after x (`head` elements before it and the `tail` elements after the last
//     whole vector are taken element-wise by workgroup 0).  A lane issues kUnroll = 4 independent 16-byte loads per trip
//     (16 KiB per workgroup, 64 KiB per CU at four resident workgroups), folds them into its private accumulator ACC, and
//     the workgroup reduces the accumulators in a fixed order (shuffle-down tree per wave, waves 0..3 in order) into ONE
//     slab of 8-byte slots.  No global atomics; LDS integer atomics only for histogram bins of more than kRegBins bins.
// (b) onehot_kernel<T>: every workgroup owns a contiguous range of rows; a row is read as 16-byte aligned blocks by
//     W = min(64, pow2 >= blocks per row) adjacent lanes (64 / W rows per wave step, kUnroll steps' loads in flight), its sum
//     and sign are reduced inside those W lanes, and a good row adds 1 to the LDS bin of its only non-zero column.
// (c) combine_kernel / combine_normal_kernel: the slabs in range order -> the statistics block.
//
// The normal family is ONE pass and never forms raw moments.  Every value is first shifted by the sample's first value
// x[0] (so that the means the pass carries are of the size of the spread, not of the size of the data: the pairwise
// update is first order in the rounding of the means it merges, and at 1e8 +- 1 unshifted means would cost eight digits of
// m2).  A lane folds each trip's shifted values (2 to 16 of them) into (k, block mean, block m2) with the block's first
// value as the base of the mean and a second sweep over the registers for the centred squares, and merges that into its
// running (n, mean, m2) by the pairwise update of Chan, Golub & LeVeque; lanes, waves and slabs merge by the same update
// in a fixed order, and the shift is added back to the mean once, at the end.  A constant sample gives m2 == 0 exactly.
// What is left of the conditioning is |mean - x[0]| / sigma in place of |mean| / sigma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace expfam {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;            // 16-byte loads in flight per lane
constexpr int kMaxSlabs = 1024;       // workgroups of a pass (four per CU), and slabs of scratch
constexpr int kMinVecs = 2048;        // a workgroup is given at least 32 KiB
constexpr int kRegBins = 8;           // histograms of up to this many bins live in registers (no same-address LDS atomics)
constexpr int kLgammaTable = 256;     // lgamma(k + 1), k < 256, per workgroup in LDS

// (out of line: the library routine's registers would otherwise set the streaming loop's occupancy)
__device__ __attribute__((noinline)) double lgamma_call(double x) { return lgamma(x); }

// An empty statement that reads all of a trip's loaded registers: the compiler cannot sink a load below it, so the kUnroll
// loads are issued back to back before the first value is used.
__device__ inline void issued(uint4 (&q)[kUnroll]) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) asm volatile("" : "+v"(q[u].x), "+v"(q[u].y), "+v"(q[u].z), "+v"(q[u].w));
}

struct Reduce {
    int64_t* red_i;
    double* red_d;
};

template <typename V, typename Op>
__device__ inline V block_reduce(V v, V* red, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    V r = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = op(r, red[w]);
    return r;
}
__device__ inline int64_t block_sum(int64_t v, const Reduce& r) {
    return block_reduce<long long>((long long)v, (long long*)r.red_i, [](long long a, long long b) { return a + b; });
}
__device__ inline int64_t block_max(int64_t v, const Reduce& r) {
    return block_reduce<long long>((long long)v, (long long*)r.red_i, [](long long a, long long b) { return a > b ? a : b; });
}
__device__ inline double block_sum(double v, const Reduce& r) {
    return block_reduce<double>(v, r.red_d, [](double a, double b) { return a + b; });
}
__device__ inline int64_t as_slot(double v) { return (int64_t)__double_as_longlong(v); }
__device__ inline double as_double(int64_t v) { return __longlong_as_double((long long)v); }

struct Moments {
    double n, mean, m2;
};
__device__ inline Moments merge(const Moments& a, const Moments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean, r = b.n / n;
    return Moments{n, a.mean + d * r, a.m2 + b.m2 + d * d * a.n * r};
}
__device__ inline Moments shfl_down(const Moments& m, int off) {
    return Moments{__shfl_down(m.n, off), __shfl_down(m.mean, off), __shfl_down(m.m2, off)};
}

// ---- accumulators: init (cooperative, before a barrier), block<K> (K values of one trip), finish (slab) --------------------
template <typename T>
struct BernoulliAcc {
    static constexpr int kSlab = 3;         // bad, n1, n0
    int64_t bad = 0, n1 = 0, n0 = 0;
    static __host__ __device__ int slab_len(int) { return kSlab; }
    static __host__ __device__ size_t lds_bytes(int) { return 0; }
    __device__ void init(unsigned char*, int, const T*) {}
    template <int K>
    __device__ void block(const T (&v)[K]) {
        unsigned b = 0, c1 = 0, c0 = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c1 += v[k] == (T)1;
            c0 += v[k] == (T)0;
            b += (v[k] != (T)0) & (v[k] != (T)1);
        }
        bad += b, n1 += c1, n0 += c0;
    }
    __device__ void finish(int64_t* slab, int, const Reduce& r) {
        const int64_t sb = block_sum(bad, r), s1 = block_sum(n1, r), s0 = block_sum(n0, r);
        if (threadIdx.x == 0) slab[0] = sb, slab[1] = s1, slab[2] = s0;
    }
};

template <typename T, bool REG>
struct CountsAcc {
    int64_t bad = 0, mx = INT64_MIN;
    unsigned long long* bins = nullptr;
    int64_t c[REG ? kRegBins : 1] = {};
    int degree = 0;
    static __host__ __device__ int slab_len(int degree) { return 2 + degree; }      // bad, max, counts
    static __host__ __device__ size_t lds_bytes(int degree) { return REG ? 0 : sizeof(unsigned long long) * (size_t)degree; }
    __device__ void init(unsigned char* lds, int degree_, const T*) {
        degree = degree_;
        if constexpr (!REG) {
            bins = (unsigned long long*)lds;
            for (int j = threadIdx.x; j < degree; j += kThreads) bins[j] = 0ull;
        }
    }
    template <int K>
    __device__ void block(const T (&v)[K]) {
        unsigned b = 0, cc[REG ? kRegBins : 1] = {};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t w = (int64_t)v[k];
            mx = w > mx ? w : mx;
            const bool ok = (uint64_t)w < (uint64_t)degree;        // a bad value is never an index
            b += !ok;
            if constexpr (REG) {
#pragma unroll
                for (int j = 0; j < kRegBins; ++j) cc[j] += ok & (w == j);
            } else {
                if (ok) atomicAdd(&bins[w], 1ull);
            }
        }
        bad += b;
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < kRegBins; ++j) c[j] += cc[j];
        }
    }
    __device__ void finish(int64_t* slab, int, const Reduce& r) {
        const int64_t sb = block_sum(bad, r), sm = block_max(mx, r);
        if (threadIdx.x == 0) slab[0] = sb, slab[1] = sm;
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < kRegBins; ++j) {
                const int64_t s = block_sum(c[j], r);
                if (threadIdx.x == 0 && j < degree) slab[2 + j] = s;
            }
        } else {
            __syncthreads();
            for (int j = threadIdx.x; j < degree; j += kThreads) slab[2 + j] = (int64_t)bins[j];
        }
    }
};

template <typename T>
struct PoissonAcc {
    static constexpr int kSlab = 3;         // bad, sum, sum_lgamma
    int64_t bad = 0, sum = 0;
    double slg = 0.0;
    const double* tab = nullptr;
    static __host__ __device__ int slab_len(int) { return kSlab; }
    static __host__ __device__ size_t lds_bytes(int) { return sizeof(double) * kLgammaTable; }
    __device__ void init(unsigned char* lds, int, const T*) {
        double* t = (double*)lds;
        for (int j = threadIdx.x; j < kLgammaTable; j += kThreads) t[j] = lgamma_call((double)j + 1.0);
        tab = t;
    }
    template <int K>
    __device__ void block(const T (&v)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t w = (int64_t)v[k];
            if (w < 0) {
                ++bad;
            } else {
                sum += w;
                slg += w < kLgammaTable ? tab[w] : lgamma_call((double)w + 1.0);
            }
        }
    }
    __device__ void finish(int64_t* slab, int, const Reduce& r) {
        const int64_t sb = block_sum(bad, r), ss = block_sum(sum, r);
        const double sl = block_sum(slg, r);
        if (threadIdx.x == 0) slab[0] = sb, slab[1] = ss, slab[2] = as_slot(sl);
    }
};

template <typename T>
struct ExponentialAcc {
    static constexpr int kSlab = 2;         // bad, sum
    int64_t bad = 0;
    double sum = 0.0;
    static __host__ __device__ int slab_len(int) { return kSlab; }
    static __host__ __device__ size_t lds_bytes(int) { return 0; }
    __device__ void init(unsigned char*, int, const T*) {}
    template <int K>
    __device__ void block(const T (&v)[K]) {
        unsigned b = 0;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool ok = v[k] > (T)0;        // false for NaN, 0 and -0.0
            b += !ok;
            s += ok ? (double)v[k] : 0.0;
        }
        bad += b, sum += s;
    }
    __device__ void finish(int64_t* slab, int, const Reduce& r) {
        const int64_t sb = block_sum(bad, r);
        const double ss = block_sum(sum, r);
        if (threadIdx.x == 0) slab[0] = sb, slab[1] = as_slot(ss);
    }
};

template <typename T>
struct NormalAcc {
    static constexpr int kSlab = 4;         // n, mean - shift, m2, shift (all binary64 in the slab)
    Moments m{0.0, 0.0, 0.0};
    double shift = 0.0;
    static __host__ __device__ int slab_len(int) { return kSlab; }
    static __host__ __device__ size_t lds_bytes(int) { return 0; }
    __device__ void init(unsigned char*, int, const T* x) { shift = (double)x[0]; }
    template <int K>
    __device__ void block(const T (&v)[K]) {
        const double y0 = (double)v[0] - shift;
        double s = 0.0;
#pragma unroll
        for (int k = 1; k < K; ++k) s += ((double)v[k] - shift) - y0;
        const double bm = y0 + s * (1.0 / K);       // K is a power of two
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double e = ((double)v[k] - shift) - bm;
            m2 += e * e;
        }
        m = merge(m, Moments{(double)K, bm, m2});
    }
    __device__ void finish(int64_t* slab, int, const Reduce& r) {
        Moments a = m;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a = merge(a, shfl_down(a, off));
        __shared__ Moments wm[kWaves];
        if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            Moments t = wm[0];
            for (int w = 1; w < kWaves; ++w) t = merge(t, wm[w]);
            slab[0] = as_slot(t.n), slab[1] = as_slot(t.mean), slab[2] = as_slot(t.m2), slab[3] = as_slot(shift);
        }
    }
};

// ---- (a) ------------------------------------------------------------------------------------------------------------------
template <typename T, typename ACC>
__global__ __launch_bounds__(kThreads) void stream_kernel(const T* __restrict__ x, int64_t n, int64_t head, int64_t nvec,
                                                          int64_t vps, int degree, int64_t* __restrict__ work) {
    constexpr int V = 16 / sizeof(T);
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int64_t red_i[kWaves];
    __shared__ double red_d[kWaves];
    const Reduce red{red_i, red_d};
    ACC acc;
    acc.init(lds, degree, x);
    __syncthreads();

    const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x + head);
    const int64_t lo = (int64_t)blockIdx.x * vps;
    const int64_t hi = lo + vps < nvec ? lo + vps : nvec;
    int64_t i = lo + threadIdx.x;
    for (; i + (kUnroll - 1) * kThreads < hi; i += kUnroll * kThreads) {
        uint4 q[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) q[u] = xv[i + u * kThreads];
        issued(q);
        T v[kUnroll * V];
        __builtin_memcpy(v, q, sizeof q);
        acc.template block<kUnroll * V>(v);
    }
    for (; i < hi; i += kThreads) {
        const uint4 q = xv[i];
        T v[V];
        __builtin_memcpy(v, &q, sizeof q);
        acc.template block<V>(v);
    }
    if (blockIdx.x == 0) {      // fewer than V elements before the first and after the last whole vector
        if ((int64_t)threadIdx.x < head) {
            const T v[1] = {x[threadIdx.x]};
            acc.template block<1>(v);
        }
        const int64_t t = head + nvec * V + threadIdx.x;
        if (t < n) {
            const T v[1] = {x[t]};
            acc.template block<1>(v);
        }
    }
    acc.finish(work + (int64_t)blockIdx.x * ACC::slab_len(degree), degree, red);
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
// Rows are read as the 16-byte ALIGNED blocks of memory that hold a part of them (a block's other bytes belong to the
// neighbouring rows or to the padding between rows and are masked out by column index; an aligned block never leaves the
// page its row bytes are on).  W = min(64, pow2 >= blocks per row) adjacent lanes own a row, 64 / W rows per wave step, and a
// wave issues the loads of kUnroll such steps before it unpacks any of them.
template <typename T>
__global__ __launch_bounds__(kThreads) void onehot_kernel(const T* __restrict__ x, int64_t n, int degree, int64_t ld, int W,
                                                          int64_t rps, int64_t* __restrict__ work) {
    constexpr int V = 16 / sizeof(T);
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int64_t red_i[kWaves];
    __shared__ double red_d[kWaves];
    const Reduce red{red_i, red_d};
    unsigned long long* bins = (unsigned long long*)lds;
    for (int j = threadIdx.x; j < degree; j += kThreads) bins[j] = 0ull;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / W;                     // rows of a wave step
    const int sub = lane / W, c0 = lane & (W - 1);
    const int64_t lo = (int64_t)blockIdx.x * rps;
    const int64_t hi = lo + rps < n ? lo + rps : n;
    const int trips = ((V - 1 + degree + V - 1) / V + W - 1) / W;       // blocks of the worst-aligned row, over W lanes
    const uintptr_t xb = (uintptr_t)x;
    int64_t bad = 0;
    for (int64_t base = lo + (int64_t)wave * rpw; base < hi; base += (int64_t)kWaves * rpw * kUnroll) {   // wave-uniform
        const uint4* blk[kUnroll];      // first aligned block of the row
        int skip[kUnroll], nblk[kUnroll];   // elements of that block before the row; blocks of the row
        long long sum[kUnroll];
        int neg[kUnroll], hit[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t r = base + (int64_t)u * kWaves * rpw + sub;
            const int64_t off = r * ld * (int64_t)sizeof(T);
            const int mis = (int)((xb + (uintptr_t)off) & 15);
            blk[u] = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(x) + (off - mis));
            skip[u] = mis / (int)sizeof(T);
            nblk[u] = r < hi ? (skip[u] + degree + V - 1) / V : 0;
            sum[u] = 0, neg[u] = 0, hit[u] = -1;
        }
        for (int t = 0; t < trips; ++t) {
            const int j = c0 + t * W;
            uint4 q[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) q[u] = j < nblk[u] ? blk[u][j] : uint4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                T v[V];
                __builtin_memcpy(v, &q[u], sizeof(uint4));
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int c = j * V + e - skip[u];
                    const bool in = j < nblk[u] && c >= 0 && c < degree;
                    const int64_t w = in ? (int64_t)v[e] : 0;
                    neg[u] |= w < 0;
                    sum[u] += w;
                    hit[u] = w != 0 ? c : hit[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            for (int off = W >> 1; off > 0; off >>= 1) {
                sum[u] += __shfl_xor(sum[u], off);
                neg[u] |= __shfl_xor(neg[u], off);
            }
            const bool active = nblk[u] > 0;
            const bool ok = active && !neg[u] && sum[u] == 1;
            // a good row has exactly one non-zero entry and it is 1: the lane that saw it owns the row's count
            if (ok && hit[u] >= 0) atomicAdd(&bins[hit[u]], 1ull);
            bad += active && !ok && c0 == 0;
        }
    }
    const int64_t sb = block_sum(bad, red);
    int64_t* slab = work + (int64_t)blockIdx.x * (1 + degree);
    if (threadIdx.x == 0) slab[0] = sb;
    __syncthreads();
    for (int j = threadIdx.x; j < degree; j += kThreads) slab[1 + j] = (int64_t)bins[j];
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
// out[0] = n, out[1 + j] = slot j of the S slabs combined in slab order: the maximum for j == max_slot, a binary64 sum for
// j == dsum_slot, an int64 sum otherwise.
__global__ __launch_bounds__(kThreads) void combine_kernel(const int64_t* __restrict__ work, int S, int slab_len, int64_t n,
                                                           int max_slot, int dsum_slot, int64_t* __restrict__ out) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j == 0) out[0] = n;
    if (j >= slab_len) return;
    if (j == dsum_slot) {
        double s = 0.0;
        for (int b = 0; b < S; ++b) s += as_double(work[(int64_t)b * slab_len + j]);
        out[1 + j] = as_slot(s);
    } else if (j == max_slot) {
        int64_t m = INT64_MIN;
        for (int b = 0; b < S; ++b) {
            const int64_t v = work[(int64_t)b * slab_len + j];
            m = v > m ? v : m;
        }
        out[1 + j] = m;
    } else {
        int64_t s = 0;
        for (int b = 0; b < S; ++b) s += work[(int64_t)b * slab_len + j];
        out[1 + j] = s;
    }
}

// One wave: lane l merges its run of consecutive slabs in order, then the lanes merge in a shuffle-down tree.
__global__ __launch_bounds__(64) void combine_normal_kernel(const int64_t* __restrict__ work, int S, int64_t n,
                                                            int64_t* __restrict__ out) {
    const int per = (S + 63) / 64;
    Moments a{0.0, 0.0, 0.0};
    for (int b = threadIdx.x * per; b < (int)(threadIdx.x + 1) * per && b < S; ++b)
        a = merge(a, Moments{as_double(work[4 * b]), as_double(work[4 * b + 1]), as_double(work[4 * b + 2])});
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = merge(a, shfl_down(a, off));
    if (threadIdx.x == 0) out[0] = n, out[1] = as_slot(as_double(work[3]) + a.mean), out[2] = as_slot(a.m2);
}

}  // namespace expfam
