// Kernels of include/ctree.h: the deepest-level count, the per-level up-sweep and the per-level MAP sweep of a context tree.
//
// Keys: a node at depth d is the context (x[i-1], ..., x[i-d]) with key sum_j x[i-j] k^(j-1); child c of key s has key
// s + c k^d one level down, so the k children of ADJACENT keys are k runs of adjacent keys and every child read below is
// coalesced when adjacent keys go to adjacent lanes.
//
// (a) count_kernel<T, LDSH>: every workgroup (256 threads) owns a contiguous range of i; lane i reads x[i] and the D symbols
//     before it (the halo of the range's first samples lies in the previous workgroup's range), so adjacent lanes read
//     adjacent symbols at every step.  LDSH: the k^(D+1) <= 4096 int64 bins are a workgroup-private LDS histogram (LDS
//     integer atomics, exact and order-free) written out as one slab per workgroup; count_combine_kernel adds the slabs in
//     range order.  Otherwise: 64-bit integer global atomics into the zeroed table.  No floating-point atomics anywhere.
//     A symbol outside 0..k-1 is counted in `bad`, never multiplied into a key, and the index is checked against the table
//     once more before the add.
// (b) sweep_deepest_kernel / sweep_level_kernel: one launch per level D, D-1, ..., 0, one lane per key.  A level's kernel
//     forms its counts as child sums (+ the head sample), then the Dirichlet-multinomial ratio and the two-way mixture of
//     DESIGN.md "Context tree".  A node whose counts are all zero returns before it writes any state.
// (c) map_level_kernel: the same level structure for the MAP recursion.
// The non-template kernels are `static`: ctsp_kernels.h includes this header for the node arithmetic, in a second
// translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ctree {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSlabs = 1024;       // workgroups of the count (four per CU), and slabs of scratch
constexpr int kMinSpan = 4096;        // a workgroup is given at least this many samples

// (out of line: the library routine's registers would otherwise set every caller's occupancy)
__device__ __attribute__((noinline)) double lgamma_call(double x) { return lgamma(x); }

__device__ inline bool in_alphabet(int64_t v, int k) { return (uint64_t)v < (uint64_t)k; }

// ---- (a) ------------------------------------------------------------------------------------------------------------------
template <typename T, bool LDSH>
__global__ __launch_bounds__(kThreads) void count_kernel(const T* __restrict__ x, int64_t n, int64_t span, int k, int D,
                                                         int64_t bins, unsigned long long* __restrict__ table,
                                                         int64_t* __restrict__ work) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ long long red[kWaves];
    unsigned long long* h = LDSH ? (unsigned long long*)lds : table;
    if (LDSH) {
        for (int64_t j = threadIdx.x; j < bins; j += kThreads) h[j] = 0ull;
        __syncthreads();
    }
    const int64_t lo = (int64_t)blockIdx.x * span;
    const int64_t hi = lo + span < n ? lo + span : n;
    long long bad = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
        const int64_t a = (int64_t)x[i];
        const bool ok = in_alphabet(a, k);
        bad += !ok;
        if (!ok || i < D) continue;
        bool valid = true;
        uint32_t key = 0, mul = 1;         // key < k^D <= 2^24
        for (int j = 1; j <= D; ++j) {
            const int64_t s = (int64_t)x[i - j];
            if (!in_alphabet(s, k)) {
                valid = false;
                break;
            }
            key += (uint32_t)s * mul;
            mul *= (uint32_t)k;
        }
        const int64_t idx = (int64_t)key * k + a;
        if (valid && idx < bins) atomicAdd(&h[idx], 1ull);
    }
    // the workgroup's `bad`: shuffle-down tree per wave, waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    const int64_t slab_len = LDSH ? 1 + bins : 1;
    int64_t* slab = work + (int64_t)blockIdx.x * slab_len;
    if (threadIdx.x == 0) {
        long long s = red[0];
        for (int w = 1; w < kWaves; ++w) s += red[w];
        slab[0] = s;
    }
    if (LDSH)
        for (int64_t j = threadIdx.x; j < bins; j += kThreads) slab[1 + j] = (int64_t)h[j];
}

// out = [ n | bad | table ]: slot 1 + j of the S slabs added in slab order.  The global-atomic path has slab_len = 1 (only
// `bad`) and its table is already in place.
static __global__ __launch_bounds__(kThreads) void count_combine_kernel(const int64_t* __restrict__ work, int S,
                                                                        int64_t slab_len, int64_t n,
                                                                        int64_t* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j == 0) out[0] = n;
    if (j >= slab_len) return;
    int64_t s = 0;
    for (int b = 0; b < S; ++b) s += work[(int64_t)b * slab_len + j];
    out[1 + j] = s;
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
// lnDM(b', n') of a row whose prior is b0 (+ 1 at `hs` when hs >= 0) and whose counts are c (- 1 at `hs`), and beta <- b0 + c.
// Sums run a = 0..k-1 in order.
//
// lnDM = G(b' + n') - G(b') with G(v) = -lnG(sum v) + sum_a lnG(v_a).  The lgamma values in G are of the size of V ln V
// (V = sum v) and cancel down to the size of V: evaluated one by one they would each carry an absolute error of an ulp of
// V ln V.  So every v_a >= kStirling, and the total, goes through Stirling's series lnG(x) = (x - 1/2) ln x - x + ln(2 pi)/2
// + t(x), in which the -x terms cancel exactly and the logarithms combine to (x - 1/2) ln(x / total): what is summed is of
// the size of the result.  Small arguments keep the library's lgamma.  A row of at most kDirect new samples (the second of
// two updates, say, on top of large b') is the rising-factorial form sum ln(b'_a + j) - sum ln(sum b' + j) itself: there
// G(b' + n') and G(b') would agree in nearly all their digits.
//
// They do the same for any batch that is small next to a prior total V = sum b' that is already in the series (an update of
// a trained model): each G is of the size of sum v ln(v / V), their difference of the size of n' ln V.  So from
// V >= kStirling on, the row is a sum of per-argument differences, in which the -n terms cancel exactly and n_a ln v_a
// joins its share n_a ln V of the total's logarithm:
//     lnG(v + n) - lnG(v) - n ln V + n = (v + n - 1/2) log1p(n / v) + n ln(v / V) + t(v + n) - t(v)          (v >= kStirling)
//     lnG(V + N) - lnG(V) - N ln V + N = (V + N - 1/2) log1p(N / V) + t(V + N) - t(V)                         (the total)
// and an argument below kStirling keeps lgamma on the side(s) where it is small:
//     (v + n - 1/2) ln((v + n) / V) + (v - 1/2) ln V - v + ln(2 pi)/2 + t(v + n) - lnG(v)              (v < kStirling <= v + n)
//     lnG(v + n) - lnG(v) - n (ln V - 1)                                                                (v + n < kStirling)
// Every term is of the size of the lnG differences it stands for (tests/test_gpu_contexttree_rows.py holds the sweep to
// 64 eps of their sum against an exact evaluation).  A first update from a small prior (V < kStirling) keeps
// G(b' + n') - G(b').
constexpr double kStirling = 64.0;        // t(x) below is exact to 1e-18 from here on
constexpr int kDirect = 64;
__device__ inline double stirling_tail(double x) {
    const double r = 1.0 / x, r2 = r * r;
    return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
}

// One side of G: feed every v_a to add(), then value().
struct LogBeta {
    double total, small = 0.0, big = 0.0, rest = 0.0;      // lgamma terms; series terms; sum of the v that stay with lgamma
    int m = 0;                                              // number of v in the series
    __device__ explicit LogBeta(double total_) : total(total_) {}
    __device__ void add(double v) {
        if (total >= kStirling && v >= kStirling) {
            const double r = v / total;
            big += (v - 0.5) * (r > 0.5 ? log1p(-(total - v) / total) : log(r)) + stirling_tail(v);
            ++m;
        } else {
            small += lgamma_call(v);
            rest += v;
        }
    }
    __device__ double value() const {
        if (m == 0) return small - lgamma_call(total);
        const double half_ln_2pi = 0.9189385332046727;
        // -lnG(total) + sum over the series' v of lnG(v), with total = rest + sum v
        return small + big - (rest + 0.5 * (m - 1)) * log(total) + rest + (m - 1) * half_ln_2pi - stirling_tail(total);
    }
};

__device__ inline double dm_row_and_update(int k, const int64_t* __restrict__ c, double* __restrict__ b,
                                           const double* __restrict__ hn_beta, bool ex, int hs) {
    double sb = 0.0, sbn = 0.0;
    int64_t tot = 0;
    bool plain = true;          // every n'_a >= 0 (anything else is a caller's inconsistent head: no direct form)
    for (int a = 0; a < k; ++a) {
        const double b0 = ex ? b[a] : hn_beta[a];
        const double bp = a == hs ? b0 + 1.0 : b0;
        const int64_t np = a == hs ? c[a] - 1 : c[a];
        sb += bp;
        sbn += bp + (double)np;
        tot += np;
        plain = plain && np >= 0;
    }
    if (plain && tot <= kDirect) {
        double acc = 0.0;
        for (int a = 0; a < k; ++a) {
            const double b0 = ex ? b[a] : hn_beta[a];
            const double bp = a == hs ? b0 + 1.0 : b0;
            const int np = (int)(a == hs ? c[a] - 1 : c[a]);
            for (int j = 0; j < np; ++j) acc += log(bp + (double)j);
            b[a] = b0 + (double)c[a];
        }
        for (int j = 0; j < (int)tot; ++j) acc -= log(sb + (double)j);
        return acc;
    }
    if (plain && sb >= kStirling) {
        const double half_ln_2pi = 0.9189385332046727;
        const double ln_sb = log(sb);
        double acc = 0.0;
        for (int a = 0; a < k; ++a) {
            const double b0 = ex ? b[a] : hn_beta[a];
            const double bp = a == hs ? b0 + 1.0 : b0;
            const double na = (double)(a == hs ? c[a] - 1 : c[a]);
            const double v = bp + na;
            if (na > 0.0) {
                if (bp >= kStirling)
                    acc += (v - 0.5) * log1p(na / bp) + na * log(bp / sb) + (stirling_tail(v) - stirling_tail(bp));
                else if (v >= kStirling)
                    acc += (v - 0.5) * log(v / sb) + (bp - 0.5) * ln_sb - bp + half_ln_2pi + stirling_tail(v) - lgamma_call(bp);
                else
                    acc += lgamma_call(v) - lgamma_call(bp) - na * (ln_sb - 1.0);
            }
            b[a] = b0 + (double)c[a];
        }
        return acc - ((sbn - 0.5) * log1p((double)tot / sb) + (stirling_tail(sbn) - stirling_tail(sb)));
    }
    LogBeta prior(sb), post(sbn);
    for (int a = 0; a < k; ++a) {
        const double b0 = ex ? b[a] : hn_beta[a];
        const int64_t ca = c[a];
        const double bp = a == hs ? b0 + 1.0 : b0;
        prior.add(bp);
        post.add(bp + (double)(a == hs ? ca - 1 : ca));
        b[a] = b0 + (double)ca;
    }
    return post.value() - prior.value();
}

// A node above the maximal depth with at least one sample: prior weight g0, children's log-weights summed to S, head sample
// `hs` (-1: none).  beta <- beta + c; returns the new g and the node's own log-weight.  Shared with ctsp_kernels.h.
struct NodeResult {
    double g, lnw;
};
__device__ inline NodeResult inner_node_update(int k, const int64_t* __restrict__ c, double* __restrict__ b,
                                               const double* __restrict__ hn_beta, bool ex, int hs, double g0, double S) {
    double lead = 0.0;
    if (hs >= 0) {
        double sb0 = 0.0;
        for (int a = 0; a < k; ++a) sb0 += ex ? b[a] : hn_beta[a];
        lead = log((ex ? b[hs] : hn_beta[hs]) / sb0);
    }
    const double L = dm_row_and_update(k, c, b, hn_beta, ex, hs);
    double mix, gn;
    if (!(g0 > 0.0)) {
        mix = L, gn = 0.0;
    } else {
        const double A = log1p(-g0) + L, B = log(g0) + S;
        const double t = A - B;       // logaddexp(A, B)
        mix = t == 0.0 ? A + 0.6931471805599453 : t > 0.0 ? A + log1p(exp(-t)) : B + log1p(exp(t));
        // B - mix = -log1p(e^t).  Next to 1 (t < 0) that difference is known to an ulp of B only, which would cost 1 - g
        // its digits; 1 / (1 + e^t) keeps them.
        gn = t > 0.0 ? exp(B - mix) : 1.0 / (1.0 + exp(t));
    }
    return {gn, lead + mix};
}

static __global__ __launch_bounds__(kThreads) void sweep_deepest_kernel(int k, int64_t nkeys, const int64_t* __restrict__ cnt,
                                                                 double* __restrict__ beta, double* __restrict__ g,
                                                                 uint8_t* __restrict__ exists,
                                                                 const double* __restrict__ hn_beta,
                                                                 double* __restrict__ lnw) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= nkeys) return;
    const int64_t* c = cnt + s * k;
    int64_t tot = 0;
    for (int a = 0; a < k; ++a) tot += c[a];
    if (tot == 0) {
        lnw[s] = 0.0;
        return;
    }
    const bool ex = exists[s] != 0;
    lnw[s] = dm_row_and_update(k, c, beta + s * k, hn_beta, ex, -1);
    if (!ex) {
        g[s] = 0.0;
        exists[s] = 1;
    }
}

// Level d < D.  cnt_child / lnw_child are level d + 1's (k * nkeys keys); cnt, lnw, beta, g, exists are level d's.
static __global__ __launch_bounds__(kThreads) void sweep_level_kernel(int k, int d, int64_t nkeys,
                                                               const int64_t* __restrict__ cnt_child,
                                                               int64_t* __restrict__ cnt,
                                                               const double* __restrict__ lnw_child,
                                                               double* __restrict__ lnw, double* __restrict__ beta,
                                                               double* __restrict__ g, uint8_t* __restrict__ exists,
                                                               double hn_g, const double* __restrict__ hn_beta,
                                                               const int32_t* __restrict__ head, int n_head) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= nkeys) return;
    // the head sample of this level: x[d] in the context (x[d-1], ..., x[0]); it sits at one key of the level
    int hs = -1;
    if (d < n_head) {
        const int32_t a = head[d];
        bool ok = in_alphabet(a, k);
        int64_t key = 0, mul = 1;
        for (int j = 1; j <= d && ok; ++j) {
            const int32_t v = head[d - j];
            ok = in_alphabet(v, k);
            key += ok ? (int64_t)v * mul : 0;
            mul *= k;
        }
        if (ok && key == s) hs = a;
    }
    int64_t* c = cnt + s * k;
    int64_t tot = 0;
    for (int a = 0; a < k; ++a) {
        int64_t t = a == hs ? 1 : 0;
        for (int ch = 0; ch < k; ++ch) t += cnt_child[(s + (int64_t)ch * nkeys) * k + a];
        c[a] = t;
        tot += t;
    }
    if (tot == 0) {
        lnw[s] = 0.0;
        return;
    }
    double S = 0.0;
    for (int ch = 0; ch < k; ++ch) S += lnw_child[s + (int64_t)ch * nkeys];
    const bool ex = exists[s] != 0;
    const NodeResult r = inner_node_update(k, c, beta + s * k, hn_beta, ex, hs, ex ? g[s] : hn_g, S);
    g[s] = r.g;
    exists[s] = 1;
    lnw[s] = r.lnw;
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
// Level d of the MAP sweep.  pw_here = hn_g^((k^(D-d) - 1)/(k - 1) - 1) prices a missing child of a node of this level,
// pw_parent the same one level up (a missing node of this level whose parent exists).  *_child / *_parent are the
// neighbouring levels' tables (unused pointers at d = D and d = 0).
static __global__ __launch_bounds__(kThreads) void map_level_kernel(int k, int d, int D, int64_t nkeys, const double* __restrict__ g,
                                                             const uint8_t* __restrict__ exists,
                                                             const uint8_t* __restrict__ exists_child,
                                                             const double* __restrict__ val_child,
                                                             const double* __restrict__ g_parent,
                                                             const uint8_t* __restrict__ exists_parent,
                                                             double pw_here, double pw_parent, double* __restrict__ val,
                                                             uint8_t* __restrict__ map_leaf) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= nkeys) return;
    if (exists[s]) {
        if (d == D) {
            val[s] = 1.0;
            map_leaf[s] = 1;
            return;
        }
        const double gs = g[s], stop = 1.0 - gs, thr = gs * pw_here;
        double prod = 1.0;
        for (int ch = 0; ch < k; ++ch) {
            const int64_t cs = s + (int64_t)ch * nkeys;
            prod *= exists_child[cs] ? val_child[cs] : (stop > thr ? stop : thr);
        }
        const bool leaf = stop > gs * prod;
        val[s] = leaf ? stop : gs * prod;
        map_leaf[s] = leaf;
        return;
    }
    val[s] = 0.0;
    bool leaf = d == D;       // (a full subtree ends in leaves at depth D whatever the rule says)
    if (d > 0 && d < D) {
        const int64_t p = s % (nkeys / k);
        if (exists_parent[p]) {
            const double gp = g_parent[p];
            leaf = 1.0 - gp > gp * pw_parent;
        }
    }
    map_leaf[s] = leaf;
}

}  // namespace ctree
