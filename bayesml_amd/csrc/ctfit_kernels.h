// Kernels of include/ctfit.h: the context-tree update from S independent sequences ("Fit from many
// sequences").
//
// A visit is (position i, depth d <= e(i)), e(i) = min(i - start(i), D); it is a HEAD visit when d = e(i) < D, the end of a
// path that the start of its sequence cuts short.  Head h of sequence s at depth e has the fixed slot hoff[s] + e, so slots
// are in time order and every head of a later sequence has a slot >= hoff[s + 1].
//
// (a) stage_tile / locate: what the two passes over the sample share.  A tile of 256 positions and the D symbols before it
//     are staged in LDS as uint8 (a symbol outside the alphabet is counted and staged as 0: it is never an index).  Lanes 0
//     and 1 bisect seq_off for the sequences of the tile's first and last position; the slice between them is staged when
//     it has at most kSeqStage entries and every lane bisects it in LDS, otherwise the lanes bisect it in global memory.
//     Equal neighbours (empty sequences): the last s with seq_off[s] <= i.
// (b) count_kernel<T, LDSH>: a workgroup owns a range of positions.  e = D: ctree's deepest-level count (LDS histogram
//     slabs, or 64-bit global atomics).  e < D: the head's two sort keys at its slot, +1 in the upper levels' head counts
//     (64-bit integer atomics) and the node's has-heads flag.
// (c) rank_kernel<T>: every visit of depth < D whose node has heads bisects the two sorted key arrays for the first head
//     of a later sequence and adds 1 to that head's bucket (64-bit integer atomics).
// (d) scan_*: an inclusive scan of the 2H buckets in three launches; r and r_a of a head are differences of it inside
//     the head's run.
// (e) lead_short_kernel / lead_long_kernel: lead of every node with heads, over its run in time order: a serial lane up to
//     kSerialRun heads, above it a workgroup (lane l adds terms l, l + 256, ... in order, then a tree over the lanes).
// (f) sweep_level_lead_kernel: ctree's inner-node step with lead.  The deepest level is ctree::sweep_deepest_kernel.
// No floating-point atomics, no grid-wide waits; every index is range-checked before use.
#pragma once
#include "ctree_kernels.h"

namespace ctfit {

using u64 = unsigned long long;
using ctree::in_alphabet;
using ctree::kThreads;
using ctree::kWaves;

constexpr int kTile = 256;            // positions per tile: one per lane
constexpr int kMaxD = 24;             // ctree_shape: D <= 24
constexpr int kSeqStage = 512;        // entries of seq_off that a tile stages in LDS
constexpr int kSerialRun = 32;        // a run of more heads than this is summed by a workgroup
constexpr int kScanItems = 8;         // consecutive buckets per lane of the scan
constexpr int kScanTile = kThreads * kScanItems;
constexpr int kLongGrid = 1024;       // workgroups of lead_long_kernel; they stride over the long runs

struct Offsets {
    int64_t off[kMaxD + 2];           // first node of level d; off[D] = nodes of levels 0..D-1
};

// (node, slot, symbol): node < 2^24, slot < 2^31, symbol < 2^8.  Sorted: by node, then time.
__device__ inline u64 pack_time(int64_t node, int64_t slot, int a) { return ((u64)node << 40) | ((u64)slot << 8) | (u64)a; }
// (node * k + symbol, slot).  Sorted: by node, then symbol, then time.
__device__ inline u64 pack_symbol(int64_t row, int64_t slot) { return ((u64)row << 32) | (u64)slot; }

// First j in 0..H with keys[j] >= v (H when there is none).
__device__ inline int64_t lower_bound(const u64* __restrict__ keys, int64_t H, u64 v) {
    int64_t lo = 0, hi = H;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The last s in lo..hi with table[s] <= v (table ascending, table[lo] <= v).
template <typename P>
__device__ inline int64_t last_at_most(P table, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (table[mid] <= v)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// ---- (a) ------------------------------------------------------------------------------------------------------------------
struct TileStage {
    int64_t soff[kSeqStage];          // seq_off[sfirst + j]
    int64_t sfirst, slast;            // the sequences of the tile's first and last position
    uint8_t sym[kTile + kMaxD + 8];   // sym[j] = x[t0 - D + j]
};

// Stages positions t0..t1-1 (t1 - t0 <= kTile, t1 <= n) and their halo.  Every lane of the workgroup calls it; returns the
// lane's count of symbols of the tile that are outside the alphabet.
template <typename T>
__device__ inline unsigned stage_tile(TileStage& ts, const T* __restrict__ x, int64_t t0, int64_t t1, int k, int D,
                                      const int64_t* __restrict__ seq_off, int64_t S) {
    __syncthreads();                  // (the previous tile has been read)
    unsigned bad = 0;
    for (int j = threadIdx.x; j < kTile + D; j += kThreads) {
        const int64_t p = t0 - D + j;
        uint8_t s = 0;
        if (p >= 0 && p < t1) {
            const int64_t v = (int64_t)x[p];
            if (in_alphabet(v, k))
                s = (uint8_t)v;
            else if (j >= D)
                ++bad;                // (a symbol is counted by the tile that owns it)
        }
        ts.sym[j] = s;
    }
    if (threadIdx.x < 2) {
        const int64_t r = last_at_most(seq_off, (int64_t)0, S - 1, threadIdx.x == 0 ? t0 : t1 - 1);
        if (threadIdx.x == 0)
            ts.sfirst = r;
        else
            ts.slast = r;
    }
    __syncthreads();
    const int64_t m = ts.slast - ts.sfirst + 1;
    if (m <= kSeqStage)
        for (int j = threadIdx.x; j < (int)m; j += kThreads) ts.soff[j] = seq_off[ts.sfirst + j];
    __syncthreads();
    return bad;
}

// The sequence of position i of the staged tile and the depth of its context.
__device__ inline void locate(const TileStage& ts, const int64_t* __restrict__ seq_off, int64_t i, int D, int64_t* s,
                              int* e) {
    const int64_t m = ts.slast - ts.sfirst + 1;
    int64_t start;
    if (m <= kSeqStage) {
        const int64_t r = last_at_most(ts.soff, (int64_t)0, m - 1, i);
        *s = ts.sfirst + r;
        start = ts.soff[r];
    } else {
        *s = last_at_most(seq_off, ts.sfirst, ts.slast, i);
        start = seq_off[*s];
    }
    start = start < 0 ? 0 : start > i ? i : start;
    *e = (int)(i - start < (int64_t)D ? i - start : (int64_t)D);
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
// Slabs as ctree::count_kernel leaves them: [bad | histogram] per workgroup with LDSH, [bad] without.
template <typename T, bool LDSH>
__global__ __launch_bounds__(kThreads) void count_kernel(const T* __restrict__ x, int64_t n, int64_t span,
                                                         const int64_t* __restrict__ seq_off,
                                                         const int64_t* __restrict__ hoff, int64_t S, int64_t H, int k, int D,
                                                         Offsets lv, int64_t bins, u64* __restrict__ table,
                                                         int64_t* __restrict__ slabs, u64* __restrict__ key_time,
                                                         u64* __restrict__ key_symbol, u64* __restrict__ hcnt,
                                                         uint8_t* __restrict__ flag) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ TileStage ts;
    __shared__ long long red[kWaves];
    u64* h = LDSH ? (u64*)lds : table;
    if (LDSH)
        for (int64_t j = threadIdx.x; j < bins; j += kThreads) h[j] = 0ull;      // (stage_tile's barrier publishes it)
    const int64_t lo = (int64_t)blockIdx.x * span;
    const int64_t hi = lo + span < n ? lo + span : n;
    const int64_t upper = lv.off[D];
    long long bad = 0;
    for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
        const int64_t t1 = t0 + kTile < hi ? t0 + kTile : hi;
        bad += stage_tile(ts, x, t0, t1, k, D, seq_off, S);
        const int64_t i = t0 + threadIdx.x;
        if (i >= t1) continue;
        int64_t s;
        int e;
        locate(ts, seq_off, i, D, &s, &e);
        const uint8_t* ctx = ts.sym + D + threadIdx.x;      // ctx[-j] = x[i - j]; j <= e <= D stays inside the stage
        const int a = ctx[0];
        int64_t key = 0, mul = 1;                           // key < k^e <= 2^24
        for (int j = 1; j <= e; ++j) {
            key += (int64_t)ctx[-j] * mul;
            mul *= k;
        }
        if (e == D) {
            const int64_t idx = key * k + a;
            if (idx < bins) atomicAdd(&h[idx], 1ull);
            continue;
        }
        const int64_t slot = hoff[s] + e, node = lv.off[e] + key;
        if (slot < 0 || slot >= H || slot >= hoff[s + 1] || node >= upper) continue;
        key_time[slot] = pack_time(node, slot, a);
        key_symbol[slot] = pack_symbol(node * k + a, slot);
        atomicAdd(&hcnt[node * k + a], 1ull);
        flag[node] = 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    const int64_t slab_len = LDSH ? 1 + bins : 1;
    int64_t* slab = slabs + (int64_t)blockIdx.x * slab_len;
    if (threadIdx.x == 0) {
        long long t = red[0];
        for (int w = 1; w < kWaves; ++w) t += red[w];
        slab[0] = t;
    }
    if (LDSH)
        for (int64_t j = threadIdx.x; j < bins; j += kThreads) slab[1 + j] = (int64_t)h[j];
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
// One tile per workgroup.  bucket[j]: visits whose first later head of the node is entry j of sorted_time;
// bucket[H + j]: the same in sorted_symbol, among the visits that carry that entry's symbol.
template <typename T>
__global__ __launch_bounds__(kThreads) void rank_kernel(const T* __restrict__ x, int64_t n,
                                                        const int64_t* __restrict__ seq_off,
                                                        const int64_t* __restrict__ hoff, int64_t S, int64_t H, int k, int D,
                                                        Offsets lv, const u64* __restrict__ sorted_time,
                                                        const u64* __restrict__ sorted_symbol,
                                                        const uint8_t* __restrict__ flag, u64* __restrict__ bucket) {
    __shared__ TileStage ts;
    const int64_t t0 = (int64_t)blockIdx.x * kTile;
    const int64_t t1 = t0 + kTile < n ? t0 + kTile : n;
    stage_tile(ts, x, t0, t1, k, D, seq_off, S);
    const int64_t i = t0 + threadIdx.x;
    if (i >= t1) return;
    int64_t s;
    int e;
    locate(ts, seq_off, i, D, &s, &e);
    const uint8_t* ctx = ts.sym + D + threadIdx.x;
    const int a = ctx[0];
    const int top = e < D - 1 ? e : D - 1;
    const int64_t upper = lv.off[D];
    int64_t key = 0, mul = 1, later = -1;
    for (int d = 0; d <= top; ++d) {
        if (d > 0) {
            key += (int64_t)ctx[-d] * mul;
            mul *= k;
        }
        const int64_t node = lv.off[d] + key;
        if (node >= upper || flag[node] == 0) continue;
        if (later < 0) {                                    // the first slot of the sequences after this one
            later = hoff[s + 1];
            later = later < 0 ? 0 : later > H ? H : later;
        }
        const int64_t j = lower_bound(sorted_time, H, pack_time(node, later, 0));
        if (j < H && (int64_t)(sorted_time[j] >> 40) == node) atomicAdd(&bucket[j], 1ull);
        const int64_t row = node * k + a;
        const int64_t j2 = lower_bound(sorted_symbol, H, pack_symbol(row, later));
        if (j2 < H && (int64_t)(sorted_symbol[j2] >> 32) == row) atomicAdd(&bucket[H + j2], 1ull);
    }
}

// ---- (d) ------------------------------------------------------------------------------------------------------------------
// Exclusive scan of one value per lane over the workgroup; `total` receives the sum.
__device__ inline u64 block_exclusive(u64 v, u64* total) {
    __shared__ u64 buf[kThreads];
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int m = 1; m < kThreads; m <<= 1) {
        const u64 add = (int)threadIdx.x >= m ? buf[threadIdx.x - m] : 0ull;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
    }
    *total = buf[kThreads - 1];
    return buf[threadIdx.x] - v;
}

static __global__ __launch_bounds__(kThreads) void scan_sums_kernel(const u64* __restrict__ v, int64_t len,
                                                                    u64* __restrict__ tile_sum) {
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    u64 acc = 0;
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < len) acc += v[base + j];
    u64 total;
    block_exclusive(acc, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// One workgroup: tile_sum[0..tiles-1] becomes its exclusive scan.  Lane l owns a contiguous piece.
static __global__ __launch_bounds__(kThreads) void scan_tiles_kernel(u64* __restrict__ tile_sum, int64_t tiles) {
    const int64_t per = (tiles + kThreads - 1) / kThreads;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < tiles ? lo + per : tiles;
    u64 acc = 0;
    for (int64_t j = lo; j < hi; ++j) acc += tile_sum[j];
    u64 total;
    u64 run = block_exclusive(acc, &total);
    for (int64_t j = lo; j < hi; ++j) {
        const u64 t = tile_sum[j];
        tile_sum[j] = run;
        run += t;
    }
}

// v becomes its inclusive scan.
static __global__ __launch_bounds__(kThreads) void scan_apply_kernel(u64* __restrict__ v, int64_t len,
                                                                     const u64* __restrict__ tile_sum) {
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    u64 item[kScanItems], acc = 0;
    for (int j = 0; j < kScanItems; ++j) {
        item[j] = base + j < len ? v[base + j] : 0ull;
        acc += item[j];
    }
    u64 total;
    u64 run = tile_sum[blockIdx.x] + block_exclusive(acc, &total);
    for (int j = 0; j < kScanItems; ++j) {
        run += item[j];
        if (base + j < len) v[base + j] = run;
    }
}

// ---- (e) ------------------------------------------------------------------------------------------------------------------
struct LeadArgs {
    const u64* sorted_time;
    const u64* sorted_symbol;
    const u64* scan;                  // [2H], inclusive
    int64_t H;
    int k;
    const double* beta;               // all levels
    const uint8_t* exists;
    const double* hn_beta;
};

// ln((b0[a] + r_a) / (sum b0 + r)) of entry j of the run lo.. of `node`, whose prior row sums to sb0.
__device__ inline double head_term(const LeadArgs& p, int64_t node, const double* __restrict__ b0, double sb0, int64_t lo,
                                   int64_t j) {
    const u64 key = p.sorted_time[j];
    const int a = (int)(key & 0xffull);
    const int64_t slot = (int64_t)((key >> 8) & 0xffffffffull);
    if (a >= p.k) return 0.0;
    const u64 r = p.scan[j] - (lo > 0 ? p.scan[lo - 1] : 0ull);
    const int64_t row = node * p.k + a;
    const int64_t lo2 = lower_bound(p.sorted_symbol, p.H, pack_symbol(row, 0));
    const int64_t j2 = lower_bound(p.sorted_symbol, p.H, pack_symbol(row, slot));
    if (j2 >= p.H) return 0.0;
    const u64 ra = p.scan[p.H + j2] - p.scan[p.H + lo2 - 1];          // (H >= 1: the index is >= 0)
    return log((b0[a] + (double)ra) / (sb0 + (double)r));
}

__device__ inline const double* prior_row(const LeadArgs& p, int64_t node, double* sb0) {
    const double* b0 = p.exists[node] != 0 ? p.beta + node * p.k : p.hn_beta;
    double s = 0.0;
    for (int a = 0; a < p.k; ++a) s += b0[a];
    *sb0 = s;
    return b0;
}

// One lane per node of levels 0..D-1.  long_list[0] counts the long runs, long_list[1..] names their nodes.
static __global__ __launch_bounds__(kThreads) void lead_short_kernel(LeadArgs p, int64_t upper,
                                                                     const uint8_t* __restrict__ flag,
                                                                     double* __restrict__ lead, u64* __restrict__ long_list,
                                                                     int64_t long_cap) {
    const int64_t node = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (node >= upper) return;
    double acc = 0.0;
    if (flag[node] != 0) {
        const int64_t lo = lower_bound(p.sorted_time, p.H, pack_time(node, 0, 0));
        const int64_t hi = lower_bound(p.sorted_time, p.H, pack_time(node + 1, 0, 0));
        if (hi - lo > kSerialRun) {
            const u64 at = atomicAdd(&long_list[0], 1ull);
            if ((int64_t)at < long_cap) long_list[1 + at] = (u64)node;
            return;                                         // (lead_long_kernel writes lead[node])
        }
        double sb0;
        const double* b0 = prior_row(p, node, &sb0);
        for (int64_t j = lo; j < hi; ++j) acc += head_term(p, node, b0, sb0, lo, j);
    }
    lead[node] = acc;
}

static __global__ __launch_bounds__(kThreads) void lead_long_kernel(LeadArgs p, int64_t upper, double* __restrict__ lead,
                                                                    const u64* __restrict__ long_list, int64_t long_cap) {
    __shared__ double red[kThreads];
    int64_t runs = (int64_t)long_list[0];
    if (runs > long_cap) runs = long_cap;
    for (int64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t node = (int64_t)long_list[1 + r];
        if (node >= upper) continue;                        // (the same for every lane)
        const int64_t lo = lower_bound(p.sorted_time, p.H, pack_time(node, 0, 0));
        const int64_t hi = lower_bound(p.sorted_time, p.H, pack_time(node + 1, 0, 0));
        double sb0;
        const double* b0 = prior_row(p, node, &sb0);
        double acc = 0.0;
        for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) acc += head_term(p, node, b0, sb0, lo, j);
        __syncthreads();
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int m = kThreads >> 1; m > 0; m >>= 1) {
            if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
            __syncthreads();
        }
        if (threadIdx.x == 0) lead[node] = red[0];
    }
}

// ---- (f) ------------------------------------------------------------------------------------------------------------------
// Level d < D.  cnt_child / lnw_child are level d + 1's; hcnt and lead are level d's head counts and lead.
static __global__ __launch_bounds__(kThreads) void sweep_level_lead_kernel(int k, int64_t nkeys,
                                                                           const int64_t* __restrict__ cnt_child,
                                                                           const int64_t* __restrict__ hcnt,
                                                                           const double* __restrict__ lead,
                                                                           int64_t* __restrict__ cnt,
                                                                           const double* __restrict__ lnw_child,
                                                                           double* __restrict__ lnw, double* __restrict__ beta,
                                                                           double* __restrict__ g, uint8_t* __restrict__ exists,
                                                                           double hn_g, const double* __restrict__ hn_beta) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= nkeys) return;
    int64_t* c = cnt + s * k;
    int64_t tot = 0, heads = 0;
    for (int a = 0; a < k; ++a) {
        const int64_t hd = hcnt[s * k + a];
        int64_t t = hd;
        for (int ch = 0; ch < k; ++ch) t += cnt_child[(s + (int64_t)ch * nkeys) * k + a];
        c[a] = t;
        tot += t;
        heads += hd;
    }
    if (tot == 0) {
        lnw[s] = 0.0;
        return;
    }
    const bool ex = exists[s] != 0;
    double* b = beta + s * k;
    if (heads == tot) {               // head visits only: each is the reference's leaf step, which leaves g alone
        for (int a = 0; a < k; ++a) b[a] = (ex ? b[a] : hn_beta[a]) + (double)c[a];
        if (!ex) {
            g[s] = hn_g;
            exists[s] = 1;
        }
        lnw[s] = lead[s];
        return;
    }
    double S = 0.0;
    for (int ch = 0; ch < k; ++ch) S += lnw_child[s + (int64_t)ch * nkeys];
    const double g0 = ex ? g[s] : hn_g;
    const double ld = heads > 0 ? lead[s] : 0.0;
    const double L = ctree::dm_row_and_update(k, c, b, hn_beta, ex, -1) - ld;
    double mix, gn;
    if (!(g0 > 0.0)) {
        mix = L, gn = 0.0;
    } else {
        const double A = log1p(-g0) + L, B = log(g0) + S;
        const double t = A - B;       // logaddexp(A, B), and g on the side that keeps 1 - g (ctree::inner_node_update)
        mix = t == 0.0 ? A + 0.6931471805599453 : t > 0.0 ? A + log1p(exp(-t)) : B + log1p(exp(t));
        gn = t > 0.0 ? exp(B - mix) : 1.0 / (1.0 + exp(t));
    }
    g[s] = gn;
    exists[s] = 1;
    lnw[s] = ld + mix;
}

}  // namespace ctfit
