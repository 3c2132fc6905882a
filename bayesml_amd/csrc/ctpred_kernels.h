// Kernels of include/ctpred.h: the predictive distribution of every position of a held-out sample under fixed tables.
//
// Positions are independent, so there are no partitions, no scans and no state between workgroups: a position walks its own
// path.  One kernel template serves both table kinds (SPARSE) and both passes (lanes per position W = 1: the scalar pass,
// which carries only q = p[x_i]; W = ctpred_group_width(k): the vector pass, symbols across the lanes, up to four per lane).
//
// (a) rowsum_kernel: W lanes per slot, the summation order of ctpred.h, so that a visit reads one binary64 instead of k.
// (b) pass_kernel: the tile's symbols and the D before it are staged once in LDS as uint8 (a symbol outside the alphabet is
//     counted and staged as 0).  A lane finds the start of its sequence by bisection in seq_off, which gives its depth e.
//     Dense tables and the probing up-walk compute the key of depth e and walk up, one lookup per level.  The stack up-walk
//     (sparse only) probes on the way down, stops probing below the first missing node (the store keeps every ancestor of a
//     node present), and leaves the slot of every level 1..e in an LDS column of its own; a lane only ever reads what it
//     wrote itself, so the walk needs no barrier.  Either way the arithmetic is the reference's Horner form over all e + 1
//     levels, a missing node reading the default row, with contraction off so that every instantiation rounds alike.
// (c) piece_sum_kernel / seq_sum_kernel: the two fixed trees of ctpred_totals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ctpred {

using u64 = unsigned long long;

constexpr int kThreads = 256;
constexpr int kMaxLevels = 64;        // D + 1 <= 64
constexpr int kMaxPerLane = 4;        // symbols per lane of the vector pass: 256 / 64
constexpr int kPiece = 4096;
constexpr int kMaxGrid = 1 << 20;     // workgroups of the row-sum pass; it strides beyond

constexpr u64 kEmpty = ~0ull;         // include/ctsp.h: CTSP_EMPTY_KEY

__device__ inline bool in_alphabet(int64_t v, int k) { return (uint64_t)v < (uint64_t)k; }

// ctsp_kernels.h's hash and key masks (that header defines its kernels and can be included in one translation unit only).
__device__ inline u64 hash_key(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ inline u64 low_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }

// ctsp::find_or_insert without the insert: the slot of `key` in keys[0..cap-1] (cap a power of two), -1 when absent; at
// most cap steps.
__device__ inline int64_t find_only(const u64* __restrict__ keys, int64_t cap, u64 key) {
    const u64 mask = (u64)cap - 1ull;
    u64 slot = hash_key(key) & mask;
    for (int64_t step = 0; step < cap; ++step) {
        const u64 cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
        if (cur == key) return (int64_t)slot;
        if (cur == kEmpty) return -1;
        slot = (slot + 1ull) & mask;
    }
    return -1;
}

// First slot of every level (dense: off[d + 1] - off[d] = k^d; sparse: the level's capacity); off[D + 1] = all slots.
struct Levels {
    int64_t off[kMaxLevels + 1];
};

struct Tables {
    const u64* key;                   // sparse only
    const double* beta;
    const double* g;
    const uint8_t* exists;
    const double* rowsum;             // [slots + 1], the default row's sum last
};

// ---- (a) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rowsum_kernel(const u64* __restrict__ key, const uint8_t* __restrict__ exists,
                                                          const double* __restrict__ beta, int64_t slots, int has_tree,
                                                          int k, int W, const double* __restrict__ hn_beta,
                                                          double* __restrict__ rowsum) {
    const int per = kThreads / W, grp = threadIdx.x / W, sub = threadIdx.x % W;
    const int64_t first = has_tree ? 0 : slots;
    for (int64_t row = first + (int64_t)blockIdx.x * per + grp; row <= slots; row += (int64_t)gridDim.x * per) {
        const bool dflt = row == slots;
        const bool there = dflt || (exists[row] != 0 && (key == nullptr || key[row] != kEmpty));
        double s = 0.0;
        if (there) {
            const double* r = dflt ? hn_beta : beta + row * k;
            for (int j = 0; j < kMaxPerLane; ++j) {
                const int a = sub + j * W;
                if (a < k) s += r[a];
            }
        }
        for (int m = W >> 1; m > 0; m >>= 1) s += __shfl_xor(s, m, W);
        if (there && sub == 0) rowsum[row] = s;
    }
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
// Table index of the node `key` of level d, -1 when there is none.
template <bool SPARSE>
__device__ inline int64_t node_at(const Tables& t, const Levels& lv, int d, u64 key) {
    const int64_t lo = lv.off[d], cap = lv.off[d + 1] - lo;
    const int64_t s = SPARSE ? find_only(t.key + lo, cap, key) : (int64_t)key;
    if (s < 0 || s >= cap) return -1;
    return t.exists[lo + s] != 0 ? lo + s : -1;
}

template <bool SPARSE, bool STACK, typename T>
__global__ __launch_bounds__(kThreads) void pass_kernel(const T* __restrict__ x, int64_t n,
                                                        const int64_t* __restrict__ seq_off, int64_t S, int k, int b, int D,
                                                        int has_tree, Levels lv, Tables t, double hn_g,
                                                        const double* __restrict__ hn_beta, int W, int count_bad,
                                                        double* __restrict__ lnp, int64_t* __restrict__ argmax,
                                                        double* __restrict__ rows, u64* __restrict__ status) {
    static_assert(SPARSE || !STACK, "the dense walk recomputes its index and needs no stack");
    extern __shared__ unsigned char smem[];
    const int per = kThreads / W;                           // positions of this workgroup
    const int64_t base = (int64_t)blockIdx.x * per;
    uint8_t* sym = smem;                                    // sym[j] = x[base - D + j], j < per + D
    int32_t* stk = (int32_t*)(smem + ((per + D + 3) & ~3)); // STACK: [D][kThreads], level d in row d - 1

    unsigned bad = 0;
    for (int j = threadIdx.x; j < per + D; j += kThreads) {
        const int64_t i = base - D + j;
        uint8_t s = 0;
        if (i >= 0 && i < n) {
            const int64_t v = (int64_t)x[i];
            if (in_alphabet(v, k))
                s = (uint8_t)v;
            else if (j >= D)
                ++bad;                                      // (a symbol is counted by the tile that owns it)
        }
        sym[j] = s;
    }
    if (count_bad) {
        if (bad) atomicAdd(status + 1, (u64)bad);
        if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = (u64)n;
    }
    __syncthreads();

    const int grp = threadIdx.x / W, sub = threadIdx.x % W;
    const int64_t i = base + grp;
    if (i >= n) return;                                     // (a lane group leaves as one)

    int64_t start = 0;
    if (seq_off != nullptr && S > 0) {                      // the last s with seq_off[s] <= i
        int64_t lo = 0, hi = S;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (seq_off[mid] <= i)
                lo = mid;
            else
                hi = mid - 1;
        }
        start = seq_off[lo];
        start = start < 0 ? 0 : start > i ? i : start;
    }
    const int e = (int)(i - start < (int64_t)D ? i - start : (int64_t)D);
    const uint8_t* ctx = sym + D + grp;                     // ctx[-j] = x[i - j]; j <= e <= D stays inside the stage

    // down: the key of depth e, and with STACK the slots on the way
    u64 key = 0;
    int64_t slot0 = -1;
    if (STACK) {
        bool alive = has_tree != 0;
        if (alive) {
            slot0 = node_at<SPARSE>(t, lv, 0, 0);
            alive = slot0 >= 0;
        }
        for (int d = 1; d <= e; ++d) {
            key |= (u64)ctx[-d] << (b * (D - d));
            int64_t s = -1;
            if (alive) {
                s = node_at<SPARSE>(t, lv, d, key);
                alive = s >= 0;
            }
            stk[(d - 1) * kThreads + threadIdx.x] = s < 0 ? -1 : (int32_t)(s - lv.off[d]);
        }
    } else if (SPARSE) {
        for (int d = 1; d <= e; ++d) key |= (u64)ctx[-d] << (b * (D - d));
    } else {
        for (int d = 1; d <= e; ++d) key += (u64)ctx[-d] * (u64)(lv.off[d] - lv.off[d - 1]);
    }

    // up: the reference's Horner form
    const bool vec = lnp == nullptr;                        // (the scalar launch is given lnp alone, the vector launch none)
    const double hn_sum = t.rowsum[lv.off[D + 1]];
    double p[kMaxPerLane] = {0.0, 0.0, 0.0, 0.0};
    const int nsym = vec ? kMaxPerLane : 1;
    {
#pragma clang fp contract(off)
        for (int d = e; d >= 0; --d) {
            int64_t s = -1;
            if (STACK) {
                if (d == 0) {
                    s = slot0;
                } else {
                    const int32_t r = stk[(d - 1) * kThreads + threadIdx.x];
                    if (r >= 0) s = lv.off[d] + r;
                }
            } else if (has_tree) {
                s = node_at<SPARSE>(t, lv, d, key);
            }
            const double* row = s >= 0 ? t.beta + s * k : hn_beta;
            const double sum = s >= 0 ? t.rowsum[s] : hn_sum;
            const double gd = s >= 0 ? t.g[s] : (d == D ? 0.0 : hn_g);
#pragma unroll
            for (int j = 0; j < kMaxPerLane; ++j) {
                const int a = vec ? sub + j * W : (int)ctx[0];
                if (j >= nsym || a >= k) break;
                const double v = row[a];
                if (d == e) {
                    p[j] = v / sum;
                } else {
                    const double own = (1.0 - gd) * v;
                    const double below = gd * p[j];
                    p[j] = own / sum + below;
                }
            }
            if (!STACK && d > 0) {                          // the key of level d - 1
                if (SPARSE)
                    key &= ~low_mask(b * (D - d + 1));
                else
                    key -= (u64)ctx[-d] * (u64)(lv.off[d] - lv.off[d - 1]);
            }
        }
    }

    if (!vec) {
        lnp[i] = log(p[0]);
        return;
    }
    double best = -1.0;                                     // (probabilities are >= 0)
    int arg = 0x7fffffff;
    for (int j = 0; j < kMaxPerLane; ++j) {
        const int a = sub + j * W;
        if (a >= k) break;
        if (rows != nullptr) rows[i * k + a] = p[j];
        if (p[j] > best) {
            best = p[j];
            arg = a;
        }
    }
    if (argmax != nullptr) {
        for (int m = W >> 1; m > 0; m >>= 1) {              // the first maximum: the lower index wins a tie
            const double ob = __shfl_xor(best, m, W);
            const int oa = __shfl_xor(arg, m, W);
            if (ob > best || (ob == best && oa < arg)) {
                best = ob;
                arg = oa;
            }
        }
        if (sub == 0) argmax[i] = arg;
    }
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
// The last s in 0..S-1 with table[s] <= v (table ascending, table[0] = 0 <= v < table[S]).
__device__ inline int64_t last_at_most(const int64_t* __restrict__ table, int64_t S, int64_t v) {
    int64_t lo = 0, hi = S - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (table[mid] <= v)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// One workgroup per piece: lane l adds the piece's positions l, l + 256, ... in this order, then a tree over the lanes.
__global__ __launch_bounds__(kThreads) void piece_sum_kernel(const double* __restrict__ lnp, int64_t n,
                                                             const int64_t* __restrict__ seq_off,
                                                             const int64_t* __restrict__ piece_off, int64_t S,
                                                             double* __restrict__ partial) {
    __shared__ double red[kThreads];
    const int64_t piece = blockIdx.x;
    const int64_t s = last_at_most(piece_off, S, piece);
    int64_t lo = seq_off[s] + (piece - piece_off[s]) * kPiece, hi = seq_off[s + 1];
    if (hi > lo + kPiece) hi = lo + kPiece;
    if (lo < 0) lo = 0;
    if (hi > n) hi = n;
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) acc += lnp[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int m = kThreads >> 1; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[piece] = red[0];
}

// One wave per sequence: lane l adds the sequence's partials l, l + 64, ... in this order, then a tree over the lanes.
__global__ __launch_bounds__(kThreads) void seq_sum_kernel(const double* __restrict__ partial,
                                                           const int64_t* __restrict__ piece_off, int64_t S, int64_t pieces,
                                                           double* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (s >= S) return;                                     // (a wave leaves as one)
    double acc = 0.0;
    if (piece_off != nullptr) {
        int64_t lo = piece_off[s], hi = piece_off[s + 1];
        if (lo < 0) lo = 0;
        if (hi > pieces) hi = pieces;
        for (int64_t j = lo + lane; j < hi; j += 64) acc += partial[j];
    }
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) totals[s] = acc;
}

}  // namespace ctpred
