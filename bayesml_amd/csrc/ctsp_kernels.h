// Kernels of include/ctsp.h: the context-tree update and MAP sweep on per-level open-addressing hash tables.
//
// Keys are ctsp.h's: b bits per symbol, nearest symbol most significant, a level-d key keeps the top b d of the b D bits.
// `shift` below is always b (D - d) of the level in question: the number of cleared low bits of its keys.
//
// find_or_insert is the only way into a table.  Its probe sequence is bounded by the capacity; a step reads the slot's key,
// returns on a match, claims an empty slot by a 64-bit compare-and-swap (losing the race to the SAME key is a match, to
// another key a collision) or moves on.  No thread ever waits for another.  Nothing has to be initialised in a claimed slot:
// cnt and lnw are zeroed for every slot before the update, and beta, g, exists, leaf are written by the sweep, after the
// launch that claimed it.
//
// (a) count_kernel<T>: the sample ranges and the `bad` count of ctree::count_kernel; then the lanes of a wave that hold
//     the same (key, symbol) elect their lowest lane in a ballot loop of at most 64 wave-uniform steps, and only the
//     elected lanes probe and add, each its group's multiplicity.  An all-equal sample costs one atomic per wave.
// (b) levelup_kernel: one lane per (slot, symbol) of level d + 1, so a wave reads cnt contiguously; a non-zero count finds
//     or inserts the parent and adds itself to the parent's row.  Lane 0 of the grid adds the level's head sample.
// (c) sweep_kernel / map_kernel: one lane per slot.  The node arithmetic is ctree::dm_row_and_update and
//     ctree::inner_node_update, serial loops over a = 0..k-1 whose summation order is part of the result: a wave per slot
//     would need a different order and give up bit-equality with the dense engine, so wide alphabets pay strided row reads
//     instead (2 KiB apart at k = 256; profiles/ctsp.md has the cost).
// (d) find_kernel, rehash_kernel: one lane per query / per old slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctree_kernels.h"

namespace ctsp {

using ctree::in_alphabet;
using ctree::kThreads;
using ctree::kWaves;
using u64 = unsigned long long;

constexpr u64 kEmpty = ~0ull;
constexpr int kMaxSlabs = 1024;
constexpr int kMinSpan = 4096;
constexpr int kMaxLevels = 64;        // D + 1 <= 64

struct Offsets {
    int64_t off[kMaxLevels + 1];
};

__device__ inline u64 hash_key(u64 z) {      // splitmix64's finaliser: level keys differ in their high bits only
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ inline u64 low_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }

// Slot of `key` in keys[0..cap-1] (cap a power of two), -1 when absent (insert = false) or when the table is full
// (*overflow raised).  key must not be kEmpty.
__device__ inline int64_t find_or_insert(u64* __restrict__ keys, int64_t cap, u64 key, bool insert, int64_t* overflow) {
    const u64 mask = (u64)cap - 1ull;
    u64 slot = hash_key(key) & mask;
    for (int64_t step = 0; step < cap; ++step) {
        u64 cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
        if (cur == key) return (int64_t)slot;
        if (cur == kEmpty) {
            if (!insert) return -1;
            cur = atomicCAS(&keys[slot], kEmpty, key);
            if (cur == kEmpty || cur == key) return (int64_t)slot;
        }
        slot = (slot + 1ull) & mask;
    }
    if (insert) atomicMax((u64*)overflow, 1ull);
    return -1;
}

__device__ inline int64_t find_only(const u64* __restrict__ keys, int64_t cap, u64 key) {
    return find_or_insert(const_cast<u64*>(keys), cap, key, false, nullptr);
}

// Level-d key of the head sample x[d] (context head[d-1], ..., head[0]) and its symbol; false when a value is out of range.
__device__ inline bool head_key(const int32_t* __restrict__ head, int d, int k, int b, int D, u64* key, int* sym) {
    const int32_t a = head[d];
    if (!in_alphabet(a, k)) return false;
    u64 kk = 0;
    for (int j = 1; j <= d; ++j) {
        const int32_t v = head[d - j];
        if (!in_alphabet(v, k)) return false;
        kk |= (u64)v << (b * (D - j));
    }
    *key = kk;
    *sym = a;
    return true;
}

// ---- (a) ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void count_kernel(const T* __restrict__ x, int64_t n, int64_t span, int k, int b, int D,
                                                         u64* __restrict__ keys, int64_t cap, u64* __restrict__ cnt,
                                                         int64_t* __restrict__ status) {
    __shared__ long long red[kWaves];
    const int64_t lo = (int64_t)blockIdx.x * span;
    const int64_t hi = lo + span < n ? lo + span : n;
    const int lane = threadIdx.x & 63;
    long long bad = 0;
    // (every lane of a wave takes the same number of trips: the ballots below need the whole wave)
    for (int64_t base = lo; base < hi; base += kThreads) {
        const int64_t i = base + threadIdx.x;
        bool valid = false;
        u64 key = 0;
        int a = 0;
        if (i < hi) {
            const int64_t v = (int64_t)x[i];
            const bool ok = in_alphabet(v, k);
            bad += !ok;
            if (ok && i >= D) {
                valid = true;
                a = (int)v;
                for (int j = 1; j <= D; ++j) {
                    const int64_t s = (int64_t)x[i - j];
                    if (!in_alphabet(s, k)) {
                        valid = false;
                        break;
                    }
                    key |= (u64)s << (b * (D - j));
                }
            }
        }
        // equal (key, symbol) pairs of the wave: the lowest lane of each group keeps the group's size
        bool pending = valid;
        int mult = 0;
        for (u64 m = __ballot(pending); m != 0; m = __ballot(pending)) {
            const int src = __ffsll((long long)m) - 1;
            const u64 k0 = __shfl(key, src);
            const int a0 = __shfl(a, src);
            const bool same = pending && key == k0 && a == a0;
            const u64 grp = __ballot(same);
            if (lane == src) mult = __popcll(grp);
            pending = pending && !same;
        }
        if (mult > 0) {
            const int64_t slot = find_or_insert(keys, cap, key, true, status + 2);
            if (slot >= 0 && slot < cap) atomicAdd(&cnt[slot * k + a], (u64)mult);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    if (lane == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = red[0];
        for (int w = 1; w < kWaves; ++w) s += red[w];
        if (s != 0) atomicAdd((u64*)(status + 1), (u64)s);
        if (blockIdx.x == 0) status[0] = n;
    }
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
// Level d + 1 (keys_c, cap_c, cnt_c) into level d (keys, cap, cnt); shift = b (D - d).
__global__ __launch_bounds__(kThreads) void levelup_kernel(int k, int b, int D, int d, int shift,
                                                           const u64* __restrict__ keys_c, int64_t cap_c,
                                                           const u64* __restrict__ cnt_c, u64* __restrict__ keys, int64_t cap,
                                                           u64* __restrict__ cnt, const int32_t* __restrict__ head, int n_head,
                                                           int64_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t == 0 && d < n_head) {
        u64 hk;
        int hs;
        if (head_key(head, d, k, b, D, &hk, &hs)) {
            const int64_t slot = find_or_insert(keys, cap, hk, true, status + 2);
            if (slot >= 0 && slot < cap) atomicAdd(&cnt[slot * k + hs], 1ull);
        }
    }
    if (t >= cap_c * k) return;
    const u64 c = cnt_c[t];
    if (c == 0) return;
    const u64 ck = keys_c[t / k];
    if (ck == kEmpty) return;
    const u64 pk = ck & ~low_mask(shift);
    const int64_t slot = find_or_insert(keys, cap, pk, true, status + 2);
    if (slot >= 0 && slot < cap) atomicAdd(&cnt[slot * k + (int)(t % k)], c);
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
// Level d; *_c are level d + 1's (unused at d = D); shift = b (D - d).
__global__ __launch_bounds__(kThreads) void sweep_kernel(int k, int b, int D, int d, int shift, const u64* __restrict__ keys,
                                                         int64_t cap, const int64_t* __restrict__ cnt, double* __restrict__ lnw,
                                                         double* __restrict__ beta, double* __restrict__ g,
                                                         uint8_t* __restrict__ exists, uint8_t* __restrict__ leaf,
                                                         const u64* __restrict__ keys_c, int64_t cap_c,
                                                         const double* __restrict__ lnw_c, double hn_g,
                                                         const double* __restrict__ hn_beta, const int32_t* __restrict__ head,
                                                         int n_head) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= cap) return;
    const u64 key = keys[s];
    if (key == kEmpty) return;
    const int64_t* c = cnt + s * k;
    int64_t tot = 0;
    for (int a = 0; a < k; ++a) tot += c[a];
    if (tot == 0) return;          // (lnw[s] is 0 from the zeroing)
    const bool ex = exists[s] != 0;
    if (d == D) {
        lnw[s] = ctree::dm_row_and_update(k, c, beta + s * k, hn_beta, ex, -1);
        if (!ex) {
            g[s] = 0.0;
            leaf[s] = 1;
            exists[s] = 1;
        }
        return;
    }
    int hs = -1;
    if (d < n_head) {
        u64 hk;
        int a;
        if (head_key(head, d, k, b, D, &hk, &a) && hk == key) hs = a;
    }
    double S = 0.0;
    for (int ch = 0; ch < k; ++ch) {
        const int64_t cs = find_only(keys_c, cap_c, key | ((u64)ch << (shift - b)));
        if (cs >= 0 && cs < cap_c) S += lnw_c[cs];
    }
    const ctree::NodeResult r = ctree::inner_node_update(k, c, beta + s * k, hn_beta, ex, hs, ex ? g[s] : hn_g, S);
    g[s] = r.g;
    if (!ex) leaf[s] = 0;
    exists[s] = 1;
    lnw[s] = r.lnw;
}

// Level d of the MAP sweep over the existing nodes; pw_here as in ctree::map_level_kernel.
__global__ __launch_bounds__(kThreads) void map_kernel(int k, int b, int D, int d, int shift, const u64* __restrict__ keys,
                                                       int64_t cap, const double* __restrict__ g,
                                                       const uint8_t* __restrict__ exists, const u64* __restrict__ keys_c,
                                                       int64_t cap_c, const uint8_t* __restrict__ exists_c,
                                                       const double* __restrict__ val_c, double pw_here,
                                                       double* __restrict__ val, uint8_t* __restrict__ map_leaf) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= cap) return;
    const u64 key = keys[s];
    if (key == kEmpty || !exists[s]) return;
    if (d == D) {
        val[s] = 1.0;
        map_leaf[s] = 1;
        return;
    }
    const double gs = g[s], stop = 1.0 - gs, thr = gs * pw_here;
    double prod = 1.0;
    for (int ch = 0; ch < k; ++ch) {
        const int64_t cs = find_only(keys_c, cap_c, key | ((u64)ch << (shift - b)));
        const bool there = cs >= 0 && cs < cap_c && exists_c[cs];
        prod *= there ? val_c[cs] : (stop > thr ? stop : thr);
    }
    const bool is_leaf = stop > gs * prod;
    val[s] = is_leaf ? stop : gs * prod;
    map_leaf[s] = is_leaf;
}

// ---- (d) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void find_kernel(int b, int D, Offsets lv, u64* __restrict__ keys, int64_t nq,
                                                        const int32_t* __restrict__ q_level, const u64* __restrict__ q_key,
                                                        int insert, int64_t* __restrict__ slot_out,
                                                        int64_t* __restrict__ status) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= nq) return;
    const int d = q_level[q];
    const u64 key = q_key[q];
    int64_t out = -1;
    if (d >= 0 && d <= D) {
        const int used = b * D, shift = b * (D - d);
        const bool in_level = (key & low_mask(shift)) == 0 && (used >= 64 || (key >> used) == 0);
        if (in_level && key != kEmpty) {
            const int64_t cap = lv.off[d + 1] - lv.off[d];
            const int64_t slot = find_or_insert(keys + lv.off[d], cap, key, insert != 0, status + 2);
            if (slot >= 0 && slot < cap) out = lv.off[d] + slot;
        }
    }
    slot_out[q] = out;
}

// One level: old table -> new table (cleared by the caller).  Only nodes move.
__global__ __launch_bounds__(kThreads) void rehash_kernel(int k, const u64* __restrict__ keys_o, int64_t cap_o,
                                                          const double* __restrict__ beta_o, const double* __restrict__ g_o,
                                                          const uint8_t* __restrict__ exists_o,
                                                          const uint8_t* __restrict__ leaf_o, u64* __restrict__ keys_n,
                                                          int64_t cap_n, double* __restrict__ beta_n, double* __restrict__ g_n,
                                                          uint8_t* __restrict__ exists_n, uint8_t* __restrict__ leaf_n,
                                                          int64_t* __restrict__ status) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= cap_o) return;
    const u64 key = keys_o[s];
    if (key == kEmpty || !exists_o[s]) return;
    const int64_t t = find_or_insert(keys_n, cap_n, key, true, status + 2);
    if (t < 0 || t >= cap_n) return;
    for (int a = 0; a < k; ++a) beta_n[t * k + a] = beta_o[s * k + a];
    g_n[t] = g_o[s];
    leaf_n[t] = leaf_o[s];
    exists_n[t] = 1;
}

}  // namespace ctsp
