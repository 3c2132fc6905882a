// Kernels of include/ctseq.h: sequential prediction and update of a context tree for a run of m positions, level by level
// ("Sequential prediction").  Positions are local to the chunk (0..m-1, int32); `sym` holds the chunk's
// symbols and the D before it as uint8, already brought into 0..k-1, so sym[D + il - j] is x[begin + il - j].
//
// Per level d the visits of a node are one segment of perm_d (sorted by key, time order inside), and a second stable
// partition of perm_d by the symbol gives the runs of equal (symbol, key), also in time order.  Ranks inside a segment or a
// run are the counts a visit sees.  All scans run on fixed trees: one Hillis-Steele scan per workgroup of kTile positions,
// one scan of the workgroup aggregates by a single workgroup; nothing depends on the order in which workgroups run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ctseq.h"

namespace ctseq {

constexpr int kTile = CTSEQ_TILE;          // positions per workgroup, one per thread (4 waves of 64)
constexpr int kWaves = kTile / 64;
constexpr int kScanThreads = 1024;         // the single workgroup that scans tile histograms and tile aggregates
constexpr int kRowBlock = CTSEQ_ROW_BLOCK;
constexpr int kBuckets = 257;              // CTREE_MAX_K symbols and the bucket of the positions that end above the level
constexpr uint32_t kKeyBits = 24;          // a key is below CTREE_MAX_SLOTS = 2^24: (symbol << 24 | key) fits 32 bits
constexpr uint32_t kKeyMask = (1u << kKeyBits) - 1;

// ---- small device helpers ---------------------------------------------------------------------------------------------
// first index in [lo, hi) whose value is >= v (hi if none); a[] ascending
template <typename V>
__device__ inline int lower_bound(const V* a, int lo, int hi, V v) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index in [lo, hi) whose value is > v
__device__ inline int upper_bound(const uint32_t* a, int lo, int hi, uint32_t v) {
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Start of the run of equal keys that holds j, keys[0..n) ascending.  Called by every thread of a kTile workgroup with
// j = its position; lds: kTile ints.  Inside the tile an inclusive max-scan of the run starts; a run that began before the
// tile is found by bisection.
__device__ inline int run_start(const uint32_t* keys, int n, int j, int* lds) {
    const int tid = threadIdx.x;
    const bool in = j < n;
    const uint32_t kj = in ? keys[j] : 0u;
    int v = (in && (j == 0 || keys[j - 1] != kj)) ? j : -1;
    lds[tid] = v;
    __syncthreads();
    for (int off = 1; off < kTile; off <<= 1) {
        const int o = tid >= off ? lds[tid - off] : -1;
        __syncthreads();
        if (o > v) v = o;
        lds[tid] = v;
        __syncthreads();
    }
    if (in && v < 0) v = lower_bound<uint32_t>(keys, 0, j, kj);
    return v;
}

// Inclusive segmented sum over the kTile threads of a workgroup: flag = 1 starts a new segment.  On return val[tid] is the
// sum from the last start at or before tid (or from thread 0), flg[tid] whether there is a start in 0..tid.
__device__ inline void tile_segscan(double v, int f, double* val, int* flg) {
    const int tid = threadIdx.x;
    val[tid] = v;
    flg[tid] = f;
    __syncthreads();
    for (int off = 1; off < kTile; off <<= 1) {
        double pv = 0.0;
        int pf = 0;
        if (tid >= off) { pv = val[tid - off]; pf = flg[tid - off]; }
        __syncthreads();
        if (tid >= off) {
            if (!f) v = pv + v;
            f |= pf;
            val[tid] = v;
            flg[tid] = f;
        }
        __syncthreads();
    }
}

__device__ inline double sigmoid_pair(double L, double* one_minus) {
    const double e = exp(-fabs(L)), den = 1.0 + e, big = 1.0 / den, small = e / den;
    *one_minus = L >= 0.0 ? small : big;
    return L >= 0.0 ? big : small;
}

// ---- the chunk's symbols ----------------------------------------------------------------------------------------------
template <typename T>
__global__ void load_symbols_kernel(const T* __restrict__ x, int64_t n, int64_t begin, int64_t len, int k, int D,
                                    uint8_t* __restrict__ sym) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= len) return;
    const int64_t gi = begin - D + t;
    int64_t v = 0;
    if (gi >= 0 && gi < n) v = (int64_t)x[gi];
    sym[t] = (uint8_t)((v < 0 || v >= k) ? 0 : v);
}

__global__ void init_level0_kernel(int m, int* __restrict__ perm, uint32_t* __restrict__ key) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) { perm[j] = j; key[j] = 0u; }
}

// ---- stable counting partition ----------------------------------------------------------------------------------------
// BY_SYM = false: perm_{d-1} -> perm_d by the digit x[i-d]; positions with i < d go to bucket k.
// BY_SYM = true:  perm_d -> (source index, symbol << 24 | key) by the symbol x[i].
template <bool BY_SYM>
__device__ inline int digit_of(int il, int64_t begin, int d, int k, int D, const uint8_t* sym) {
    if (BY_SYM) return sym[D + il];
    return begin + il < d ? k : sym[D + il - d];
}

template <bool BY_SYM>
__global__ void part_hist_kernel(const int* __restrict__ perm, int msrc, int64_t begin, int d, int k, int D,
                                 const uint8_t* __restrict__ sym, int ntiles, int* __restrict__ hist) {
    __shared__ int h[kBuckets];
    const int tid = threadIdx.x;
    for (int b = tid; b <= k; b += kTile) h[b] = 0;
    __syncthreads();
    const int j = blockIdx.x * kTile + tid;
    if (j < msrc) atomicAdd(&h[digit_of<BY_SYM>(perm[j], begin, d, k, D, sym)], 1);
    __syncthreads();
    for (int b = tid; b <= k; b += kTile) hist[(int64_t)b * ntiles + blockIdx.x] = h[b];
}

// exclusive scan of a[0..L), in place, by ONE workgroup of kScanThreads
__global__ void scan_int_kernel(int* __restrict__ a, int64_t L) {
    __shared__ int part[kScanThreads];
    const int tid = threadIdx.x;
    const int64_t span = (L + kScanThreads - 1) / kScanThreads;
    const int64_t lo = tid * span < L ? tid * span : L, hi = lo + span < L ? lo + span : L;
    int s = 0;
    for (int64_t i = lo; i < hi; ++i) s += a[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int o = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        s += o;
        part[tid] = s;
        __syncthreads();
    }
    int run = tid ? part[tid - 1] : 0;
    for (int64_t i = lo; i < hi; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
}

template <bool BY_SYM>
__global__ void part_scatter_kernel(const int* __restrict__ perm, const uint32_t* __restrict__ key, int msrc, int64_t begin,
                                    int d, int k, int D, const uint8_t* __restrict__ sym, int ntiles,
                                    const int* __restrict__ hist, uint32_t pw_prev, int* __restrict__ operm,
                                    uint32_t* __restrict__ okey) {
    __shared__ int wcnt[kWaves][kBuckets];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int b = tid; b < kWaves * kBuckets; b += kTile) (&wcnt[0][0])[b] = 0;
    __syncthreads();
    const int j = blockIdx.x * kTile + tid;
    const bool in = j < msrc;
    const int il = in ? perm[j] : 0;
    const int dg = in ? digit_of<BY_SYM>(il, begin, d, k, D, sym) : 511;          // 511: no digit, matches nobody's
    // the lanes of this wave with the same digit
    unsigned long long same = ~0ull;
    for (int bit = 0; bit < 9; ++bit) {
        const int mine = (dg >> bit) & 1;
        const unsigned long long b = __ballot(mine);
        same &= mine ? b : ~b;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    if (in && rank == 0) wcnt[w][dg] = __popcll(same);
    __syncthreads();
    if (!in) return;
    int dst = hist[(int64_t)dg * ntiles + blockIdx.x] + rank;
    for (int ww = 0; ww < w; ++ww) dst += wcnt[ww][dg];
    if (dst < 0 || dst >= msrc) return;
    if (BY_SYM) {
        operm[dst] = j;
        okey[dst] = ((uint32_t)dg << kKeyBits) | (key[j] & kKeyMask);
    } else {
        operm[dst] = il;
        okey[dst] = key[j] + (uint32_t)dg * pw_prev;
    }
}

// ---- per level: segment starts, and what a node held before the chunk -------------------------------------------------
__global__ void seg_head_kernel(const uint32_t* __restrict__ key, int md, int d, int k, int D, uint32_t pw,
                                const double* __restrict__ beta_l, const double* __restrict__ g_l,
                                const uint8_t* __restrict__ ex_l, double hn_g, const double* __restrict__ hn_beta,
                                int* __restrict__ segst, double* __restrict__ sumb0, double* __restrict__ g0s) {
    __shared__ int lds[kTile];
    const int j = blockIdx.x * kTile + threadIdx.x;
    const int st = run_start(key, md, j, lds);
    if (j >= md) return;
    segst[j] = st;
    if (st != j) return;
    const uint32_t s = key[j];
    double sum = 1.0, g0 = 0.0;
    if (s < pw) {
        const bool ex = ex_l[s] != 0;
        const double* row = ex ? beta_l + (int64_t)s * k : hn_beta;
        sum = 0.0;
        for (int a = 0; a < k; ++a) sum += row[a];
        g0 = ex ? g_l[s] : (d == D ? 0.0 : hn_g);
    }
    sumb0[j] = sum;
    g0s[j] = g0;
}

// cA[j] = number of earlier visits of j's node with j's symbol: the rank inside the run of (symbol, key)
__global__ void sym_rank_kernel(const int* __restrict__ tmp, const uint32_t* __restrict__ tkey, int md, int* __restrict__ cA) {
    __shared__ int lds[kTile];
    const int t = blockIdx.x * kTile + threadIdx.x;
    const int rs = run_start(tkey, md, t, lds);
    if (t >= md) return;
    const int j = tmp[t];
    if (j >= 0 && j < md) cA[j] = t - rs;
}

// own estimate of the seen symbol, the log-odds step, and the tile's aggregate of the steps
__global__ void own_delta_kernel(const int* __restrict__ perm, const uint32_t* __restrict__ key, const int* __restrict__ segst,
                                 const int* __restrict__ cA, const double* __restrict__ sumb0, int md, int64_t begin, int d,
                                 int k, int D, uint32_t pw, const uint8_t* __restrict__ sym, const double* __restrict__ beta_l,
                                 const uint8_t* __restrict__ ex_l, const double* __restrict__ hn_beta,
                                 const double* __restrict__ q, double* __restrict__ own, double* __restrict__ delta,
                                 double* __restrict__ agg_sum, int* __restrict__ agg_flag) {
    __shared__ double val[kTile];
    __shared__ int flg[kTile];
    const int j = blockIdx.x * kTile + threadIdx.x;
    double dl = 0.0;
    int fl = 0;
    if (j < md) {
        const int il = perm[j], st = segst[j];
        const int a = sym[D + il];
        const uint32_t s = key[j];
        const double b0 = (s < pw && ex_l[s]) ? beta_l[(int64_t)s * k + a] : hn_beta[a];
        const double o = (b0 + (double)cA[j]) / (sumb0[st] + (double)(j - st));
        const bool end = d == D || begin + il == d;
        if (!end) dl = log(q[il]) - log(o);
        own[j] = o;
        delta[j] = dl;
        fl = st == j;
    }
    tile_segscan(dl, fl, val, flg);
    if (threadIdx.x == kTile - 1) {
        agg_sum[blockIdx.x] = val[kTile - 1];
        agg_flag[blockIdx.x] = flg[kTile - 1];
    }
}

// carry[b] = sum of the steps of the segment that runs into tile b from the tiles before it; ONE workgroup
__global__ void carry_scan_kernel(const double* __restrict__ agg_sum, const int* __restrict__ agg_flag, int nb,
                                  double* __restrict__ carry) {
    __shared__ double val[kScanThreads];
    __shared__ int flg[kScanThreads];
    const int tid = threadIdx.x;
    const int span = (nb + kScanThreads - 1) / kScanThreads;
    const int lo = tid * span < nb ? tid * span : nb, hi = lo + span < nb ? lo + span : nb;
    double v = 0.0;
    int f = 0;
    for (int b = lo; b < hi; ++b) {
        v = agg_flag[b] ? agg_sum[b] : v + agg_sum[b];
        f |= agg_flag[b];
    }
    val[tid] = v;
    flg[tid] = f;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        double pv = 0.0;
        int pf = 0;
        if (tid >= off) { pv = val[tid - off]; pf = flg[tid - off]; }
        __syncthreads();
        if (tid >= off) {
            if (!f) v = pv + v;
            f |= pf;
            val[tid] = v;
            flg[tid] = f;
        }
        __syncthreads();
    }
    double run = tid ? val[tid - 1] : 0.0;
    for (int b = lo; b < hi; ++b) {
        carry[b] = run;
        run = agg_flag[b] ? agg_sum[b] : run + agg_sum[b];
    }
}

// g before each visit, the mixed probability of the seen symbol, and the node's g after its last visit of the chunk
__global__ void mix_kernel(const int* __restrict__ perm, const uint32_t* __restrict__ key, const int* __restrict__ segst,
                           const double* __restrict__ g0s, const double* __restrict__ own, const double* __restrict__ delta,
                           const double* __restrict__ carry, int md, int64_t begin, int d, int D, uint32_t pw,
                           double* __restrict__ g_l, double* __restrict__ q, double* __restrict__ gvis) {
    __shared__ double val[kTile];
    __shared__ int flg[kTile];
    const int tid = threadIdx.x, j = blockIdx.x * kTile + tid;
    const bool in = j < md;
    const double dl = in ? delta[j] : 0.0;
    const int st = in ? segst[j] : -1;
    tile_segscan(dl, in && st == j, val, flg);
    if (!in) return;
    double excl = 0.0;                                   // the steps of the earlier visits of this node in this chunk
    if (st != j) {
        const double c = carry[blockIdx.x];
        excl = tid == 0 ? c : (flg[tid - 1] ? val[tid - 1] : c + val[tid - 1]);
    }
    const int il = perm[j];
    const double g0 = g0s[st], o = own[j];
    const bool end = d == D || begin + il == d;
    const bool fixed = !(g0 > 0.0 && g0 < 1.0);          // 0 and 1 are fixed points
    double L0 = 0.0, g = g0, omg = 1.0 - g0;
    if (!fixed) {
        L0 = log(g0) - log1p(-g0);
        if (st != j) g = sigmoid_pair(L0 + excl, &omg);
    }
    q[il] = end ? o : omg * o + g * q[il];
    gvis[j] = g;
    if (j == md - 1 || segst[j + 1] == j + 1) {          // the node's last visit
        const uint32_t s = key[j];
        if (s < pw) {
            double gout = g0, unused;
            if (!fixed && d < D && !(end && st == j)) gout = sigmoid_pair(L0 + excl + dl, &unused);
            g_l[s] = gout;
        }
    }
}

// ---- the full rows ----------------------------------------------------------------------------------------------------
// A group of W lanes (W = 64 or the power of two >= k) walks kRowBlock consecutive visits of perm_d; lane gl holds the
// symbols gl, gl + W, ... (at most 4).  The counts a node had at the block's start are ranks in the (symbol, key) runs.
__global__ void rows_level_kernel(const int* __restrict__ perm, const uint32_t* __restrict__ key, const int* __restrict__ segst,
                                  const double* __restrict__ sumb0, const double* __restrict__ gvis,
                                  const int* __restrict__ tmp, const uint32_t* __restrict__ tkey, int md, int64_t begin, int d,
                                  int k, int D, uint32_t pw, const uint8_t* __restrict__ sym, const double* __restrict__ beta_l,
                                  const uint8_t* __restrict__ ex_l, const double* __restrict__ hn_beta, int W,
                                  double* __restrict__ rows) {
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t blk = gt / W;
    const int gl = (int)(gt % W);
    if (blk * kRowBlock >= md) return;
    const int j0 = (int)(blk * kRowBlock), j1 = j0 + kRowBlock < md ? j0 + kRowBlock : md;
    double b0[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt[4] = {0, 0, 0, 0};
    int cur = -1;
    for (int j = j0; j < j1; ++j) {
        const int st = segst[j];
        if (st != cur) {
            cur = st;
            const uint32_t s = key[j];
            const bool ex = s < pw && ex_l[s];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int at = gl + t * W;
                if (at >= k) continue;
                b0[t] = ex ? beta_l[(int64_t)s * k + at] : hn_beta[at];
                cnt[t] = 0;
                if (st != j) {                           // the block starts inside the segment
                    const uint32_t c = ((uint32_t)at << kKeyBits) | (s & kKeyMask);
                    const int lo = lower_bound<uint32_t>(tkey, 0, md, c), hi = upper_bound(tkey, lo, md, c);
                    cnt[t] = lower_bound<int>(tmp, lo, hi, j) - lo;
                }
            }
        }
        const int il = perm[j];
        const int a = sym[D + il];
        const double g = gvis[j], den = sumb0[st] + (double)(j - st);
        const bool end = d == D || begin + il == d;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int at = gl + t * W;
            if (at >= k) continue;
            const double o = (b0[t] + (double)cnt[t]) / den;
            const int64_t idx = (int64_t)il * k + at;
            rows[idx] = end ? o : (1.0 - g) * o + g * rows[idx];
            if (at == a) ++cnt[t];
        }
    }
}

// ---- the tables after the chunk ---------------------------------------------------------------------------------------
__global__ void create_nodes_kernel(const uint32_t* __restrict__ key, const int* __restrict__ segst, int md, int d, int k,
                                    int D, uint32_t pw, double* __restrict__ beta_l, uint8_t* __restrict__ ex_l,
                                    uint8_t* __restrict__ leaf_l, const double* __restrict__ hn_beta) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= md || segst[j] != j) return;
    const uint32_t s = key[j];
    if (s >= pw || ex_l[s]) return;
    for (int a = 0; a < k; ++a) beta_l[(int64_t)s * k + a] = hn_beta[a];
    leaf_l[s] = d == D ? 1 : 0;
    ex_l[s] = 1;
}

__global__ void add_counts_kernel(const uint32_t* __restrict__ tkey, int md, int k, uint32_t pw, double* __restrict__ beta_l) {
    __shared__ int lds[kTile];
    const int t = blockIdx.x * kTile + threadIdx.x;
    const int rs = run_start(tkey, md, t, lds);
    if (t >= md) return;
    const uint32_t c = tkey[t];
    if (t != md - 1 && tkey[t + 1] == c) return;
    const uint32_t a = c >> kKeyBits, s = c & kKeyMask;
    if (s < pw && a < (uint32_t)k) beta_l[(int64_t)s * k + a] += (double)(t - rs + 1);
}

// ---- outputs ----------------------------------------------------------------------------------------------------------
__global__ void nats_kernel(const double* __restrict__ q, int m, double* __restrict__ nats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) nats[i] = -log(q[i]);
}

__global__ void argmax_kernel(const double* __restrict__ rows, int m, int k, int64_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double* r = rows + (int64_t)i * k;
    int best = 0;
    double bv = r[0];
    for (int a = 1; a < k; ++a)
        if (r[a] > bv) { bv = r[a]; best = a; }
    out[i] = best;
}

}  // namespace ctseq
