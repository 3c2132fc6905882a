// Kernels of include/mtgrow.h: one level of growth of every chain's proposal, and the acceptance step.
//
// (a) begin_kernel: resets the slot tables and the rows' slots.
// (b) decide_kernel: a thread per open node of the level.
// (c) first_kernel / probe_kernel<TC, TK>: a thread per (row, chain), integer atomics only.  Doubles are ordered through
//     enc(): the bit pattern with the sign handled so that unsigned order is numeric order, so atomicMin / atomicMax give
//     the exact min and max whatever the order the atomics land in.
// (d) kmeans_kernel<TC>: a workgroup per (node of the level, chain).  It walks the split feature's sorted positions
//     MTGROW_KMEANS_BLOCK at a time and keeps the positions of its node: a max-scan finds each one's predecessor in the node,
//     which makes the unique-value heads; the heads' count, x and x^2 go through fixed-order block scans with a carry from
//     tile to tile.  Pass 1 forms the totals, pass 2 the cost of every cut and its first-index argmin.
// (e) split_kernel: the leaf rule, the thresholds, the children opened.   (f) advance_kernel<TC, TK>: the rows' move.
// (g) accept_kernel: a workgroup per chain.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtgrow.h"

namespace mtgrow {

constexpr int kThreads = 256;
constexpr int kKm = MTGROW_KMEANS_BLOCK;

struct State {        // mtgrow_state by value
    int B, cap, C, dim_cont, dim_cat, max_depth, n_post, threshold;
    int64_t n;
    const void *xc, *xk;
    const int32_t* order;
    const double* draws;
    const int32_t* last_feat;
    const double* last_g;
    int32_t* feat;
    double *thr, *g, *post;
    int32_t *node, *open, *regen, *dflag, *first, *count, *differs;
    unsigned long long *lo, *hi;
    double* mid;
};

__device__ inline unsigned long long enc(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double dec(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// ---- (a) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void begin_kernel(State s, double g_root, double g_below, int last_lo,
                                                         const double* __restrict__ sub_hn) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t slots = (int64_t)s.B * s.cap;
    if (t < slots) {
        const int h = (int)(t % s.cap);
        s.feat[t] = -1;
        s.open[t] = h == 0;
        s.regen[t] = 0;
        s.dflag[t] = 0;
        s.first[t] = INT32_MAX;
        s.count[t] = 0;
        s.differs[t] = 0;
        s.lo[t] = ~0ull;
        s.hi[t] = 0ull;
        s.mid[t] = 0.0;
        s.g[t] = (h >= last_lo && s.max_depth > 0) ? 0.0 : h == 0 ? g_root : g_below;
        for (int j = 0; j < s.n_post; ++j) s.post[t * s.n_post + j] = sub_hn[j];
    }
    if (t < (int64_t)s.B * s.n) s.node[t] = 0;
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void decide_kernel(State s, int lvl_lo, int lvl_n, int all_regen, double g_max) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= lvl_n) return;
    const int h = lvl_lo + t;
    const int64_t v = (int64_t)b * s.cap + h;
    if (!s.open[v]) return;
    const int F = s.dim_cont + s.dim_cat;
    const bool regen = h == 0 ? all_regen != 0 : s.regen[(int64_t)b * s.cap + (h - 1) / s.C] != 0;
    const double u0 = s.draws[v * 2], u1 = s.draws[v * 2 + 1];
    int k, flag, re;
    if (regen) {
        k = min(F - 1, (int)floor(u1 * F));
        flag = 0;
        re = 1;
    } else {
        const int lk = s.last_feat[v];
        if (u0 > fmin(s.last_g[v], g_max)) {
            if (lk < 0 || F < 2) {        // (the last tree's node is a leaf, so this one will be: the feature is never used)
                k = min(F - 1, (int)floor(u1 * F));
            } else {
                k = min(F - 2, (int)floor(u1 * (F - 1)));
                if (k >= lk) ++k;
            }
            flag = 2;
            re = 1;
        } else {
            k = lk < 0 ? 0 : lk;
            flag = 1;
            re = 0;
        }
    }
    s.feat[v] = max(0, k);
    s.dflag[v] = flag;
    s.regen[v] = re;
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void first_kernel(State s, int lvl_lo, int lvl_hi) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= s.n) return;
    const int h = s.node[(int64_t)b * s.n + i];
    if (h < lvl_lo || h >= lvl_hi) return;
    const int64_t v = (int64_t)b * s.cap + h;
    atomicMin(&s.first[v], (int)i);
    atomicAdd(&s.count[v], 1);
}

// np.isclose(a, b) with its default tolerances, b the reference entry
__device__ inline bool close_to(double a, double b) {
    if (a == b) return true;
    if (!isfinite(a) || !isfinite(b)) return false;
    return fabs(a - b) <= 1e-8 + 1e-5 * fabs(b);
}

template <typename TC, typename TK>
__global__ __launch_bounds__(kThreads) void probe_kernel(State s, int lvl_lo, int lvl_hi) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= s.n) return;
    const int h = s.node[(int64_t)b * s.n + i];
    if (h < lvl_lo || h >= lvl_hi) return;
    const int64_t v = (int64_t)b * s.cap + h;
    const int64_t r0 = s.first[v];
    if (r0 < 0 || r0 >= s.n) return;
    const TC* xc = (const TC*)s.xc;
    const TK* xk = (const TK*)s.xk;
    bool differs = false;
    if (i != r0) {
        for (int j = 0; j < s.dim_cont && !differs; ++j)
            differs = !close_to((double)xc[i * s.dim_cont + j], (double)xc[r0 * s.dim_cont + j]);
        for (int j = 0; j < s.dim_cat && !differs; ++j)
            differs = !close_to((double)xk[i * s.dim_cat + j], (double)xk[r0 * s.dim_cat + j]);
    } else {        // a NaN in the first row is close to nothing, itself included
        for (int j = 0; j < s.dim_cont && !differs; ++j) differs = isnan((double)xc[i * s.dim_cont + j]);
    }
    if (differs) atomicOr(&s.differs[v], 1);
    const int k = s.feat[v];
    if (k >= 0 && k < s.dim_cont) {
        const double x = (double)xc[i * s.dim_cont + k];
        if (!isnan(x)) {
            const unsigned long long e = enc(x);
            atomicMin(&s.lo[v], e);
            atomicMax(&s.hi[v], e);
        }
    }
}

// ---- (d) ------------------------------------------------------------------------------------------------------------------
// Inclusive scan over the workgroup's kKm threads in thread order; `total` is the last thread's value.  Waves scan with
// shuffles, a thread then adds the totals of the waves before its own in wave order.  Ends on a barrier, so `lds` (one slot
// per wave) can be used again at once.
template <typename T, typename Op>
__device__ inline T block_scan(T v, T* lds, Op op, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v = op(t, v);
    }
    if (lane == 63) lds[w] = v;
    __syncthreads();
    T acc = lds[0];
    T mine = v;
    for (int j = 1; j < kKm / 64; ++j) {
        if (j == w) mine = op(acc, v);
        acc = op(acc, lds[j]);
    }
    total = acc;
    __syncthreads();
    return mine;
}

struct Add {
    template <typename T>
    __device__ T operator()(T a, T b) const { return a + b; }
};
struct Max {
    __device__ int operator()(int a, int b) const { return a > b ? a : b; }
};

template <typename TC>
__global__ __launch_bounds__(kKm) void kmeans_kernel(State s, int lvl_lo) {
    const int h = lvl_lo + blockIdx.x, b = blockIdx.y;
    const int64_t v = (int64_t)b * s.cap + h;
    const int k = s.feat[v];
    // uniform over the workgroup: the node splits on a continuous feature with lo < hi
    if (!s.open[v] || s.count[v] < 2 || !s.differs[v] || k < 0 || k >= s.dim_cont) return;
    if (s.lo[v] > s.hi[v] || !(dec(s.lo[v]) < dec(s.hi[v]))) return;
    const TC* xc = (const TC*)s.xc;
    const int32_t* order = s.order + (int64_t)k * s.n;
    const int32_t* node = s.node + (int64_t)b * s.n;
    __shared__ int lds_i[kKm / 64];
    __shared__ double lds_d[kKm / 64];
    __shared__ int prev_in[kKm];
    __shared__ double best_m[kKm];
    __shared__ int best_j[kKm];
    __shared__ double best_t[kKm];
    const int tid = threadIdx.x;
    double S = 0.0, Q = 0.0;
    int m = 0;
    double bm = INFINITY, bt = 0.0;
    int bj = INT32_MAX;
    for (int pass = 0; pass < 2; ++pass) {
        int carry_prev = -1, carry_n = 0;
        double carry_s = 0.0, carry_q = 0.0;
        for (int64_t base = 0; base < s.n; base += kKm) {
            const int64_t p = base + tid;
            bool in = false;
            double x = 0.0;
            if (p < s.n) {
                const int64_t r = order[p];
                if (r >= 0 && r < s.n && node[r] == h) {
                    x = (double)xc[r * s.dim_cont + k];
                    in = !isnan(x);
                }
            }
            int tot_i;
            const int incl = max(carry_prev, block_scan<int>(in ? (int)p : -1, lds_i, Max(), tot_i));
            prev_in[tid] = incl;
            __syncthreads();
            const int before = tid > 0 ? prev_in[tid - 1] : carry_prev;
            carry_prev = max(carry_prev, tot_i);
            double xp = 0.0;
            if (in && before >= 0) xp = (double)xc[(int64_t)order[before] * s.dim_cont + k];
            const bool head = in && (before < 0 || xp != x);
            int tot_n;
            double tot_s, tot_q;
            const int jn = block_scan<int>(head ? 1 : 0, lds_i, Add(), tot_n);
            const double js = block_scan<double>(head ? x : 0.0, lds_d, Add(), tot_s);
            const double jq = block_scan<double>(head ? x * x : 0.0, lds_d, Add(), tot_q);
            if (pass == 1 && head) {
                const int j = carry_n + jn - 1;        // unique values before this one
                if (j >= 1) {
                    const double sl = carry_s + (js - x), ql = carry_q + (jq - x * x);
                    const double sr = S - sl, qr = Q - ql;
                    const double metric = (ql - sl * sl / j) + (qr - sr * sr / (m - j));
                    if (metric < bm) {
                        bm = metric;
                        bj = j;
                        bt = (xp + x) / 2;
                    }
                }
            }
            carry_n += tot_n;
            carry_s += tot_s;
            carry_q += tot_q;
        }
        if (pass == 0) {
            m = carry_n;
            S = carry_s;
            Q = carry_q;
            if (m < 2) return;        // uniform
        }
    }
    best_m[tid] = bm;
    best_j[tid] = bj;
    best_t[tid] = bt;
    __syncthreads();
    for (int off = kKm / 2; off > 0; off >>= 1) {
        if (tid < off) {
            const double om = best_m[tid + off];
            const int oj = best_j[tid + off];
            if (om < best_m[tid] || (om == best_m[tid] && oj < best_j[tid])) {
                best_m[tid] = om;
                best_j[tid] = oj;
                best_t[tid] = best_t[tid + off];
            }
        }
        __syncthreads();
    }
    if (tid == 0) s.mid[v] = best_t[0];
}

// ---- (e) ------------------------------------------------------------------------------------------------------------------
// a + j * d with the product rounded before the sum (the compiler would otherwise fuse the two)
__device__ inline double add_product(double a, double j, double d) {
#pragma clang fp contract(off)
    const double p = j * d;
    return a + p;
}

__global__ __launch_bounds__(kThreads) void split_kernel(State s, int lvl_lo, int lvl_n) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= lvl_n) return;
    const int h = lvl_lo + t;
    const int64_t v = (int64_t)b * s.cap + h;
    if (!s.open[v]) return;
    if (s.count[v] == 0 || !s.differs[v]) {        // an empty child keeps its prior g; a node of identical rows is a leaf
        s.feat[v] = -1;
        s.dflag[v] = 0;
        s.regen[v] = 1;
        if (s.count[v] > 0) s.g[v] = 0.0;
        return;
    }
    const int k = s.feat[v], C = s.C;
    if (k < s.dim_cont) {
        double* thr = s.thr + v * (C + 1);
        // every row NaN in feature k: no min; the rows all stay here
        const bool none = s.lo[v] > s.hi[v];
        const double lo = none ? NAN : dec(s.lo[v]), hi = none ? NAN : dec(s.hi[v]);
        if (!(lo < hi)) {
            for (int j = 0; j <= C; ++j) thr[j] = lo;
        } else if (s.threshold == MTGROW_KMEANS && C == 2) {
            thr[0] = lo;
            thr[1] = s.mid[v];
            thr[2] = hi;
        } else {
            // NumPy's fill: the product and the sum are rounded separately (no fused multiply-add)
            const double w = (hi - lo) / C, delta = (lo + w) - lo;
            for (int j = 0; j <= C; ++j) thr[j] = j == 0 ? lo : j == 1 ? lo + w : add_product(lo, (double)j, delta);
        }
    }
    const int64_t c0 = (int64_t)b * s.cap + (int64_t)C * h + 1;
    if ((int64_t)C * h + C < s.cap)
        for (int j = 0; j < C; ++j) s.open[c0 + j] = 1;
}

// ---- (f) ------------------------------------------------------------------------------------------------------------------
template <typename TC, typename TK>
__global__ __launch_bounds__(kThreads) void advance_kernel(State s, int lvl_lo, int lvl_hi) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= s.n) return;
    const int h = s.node[(int64_t)b * s.n + i];
    if (h < lvl_lo || h >= lvl_hi) return;
    const int64_t v = (int64_t)b * s.cap + h;
    const int k = s.feat[v], C = s.C;
    if (k < 0 || (int64_t)C * h + C >= s.cap) return;
    int child = -1;
    if (k < s.dim_cont) {
        const double* thr = s.thr + v * (C + 1);
        const double x = (double)((const TC*)s.xc)[i * s.dim_cont + k];
        if (x < thr[1]) child = 0;
        else if (thr[C - 1] <= x) child = C - 1;
        else
            for (int j = 1; j + 1 < C; ++j)
                if (thr[j] <= x && x < thr[j + 1]) {
                    child = j;
                    break;
                }
    } else {
        const int64_t a = (int64_t)((const TK*)s.xk)[i * s.dim_cat + (k - s.dim_cont)];
        if ((uint64_t)a < (uint64_t)C) child = (int)a;
    }
    if (child >= 0) s.node[(int64_t)b * s.n + i] = C * h + 1 + child;
}

// ---- (g) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void accept_kernel(State s, int tempered, double g_max, const double* __restrict__ l_new,
                                                          double* __restrict__ l_last, const double* __restrict__ beta,
                                                          const double* __restrict__ u, const double* __restrict__ lml,
                                                          const double* __restrict__ lcm, int32_t* __restrict__ last_feat,
                                                          double* __restrict__ last_thr, double* __restrict__ last_g,
                                                          double* __restrict__ last_post, double* __restrict__ last_lml,
                                                          double* __restrict__ last_lcm, double* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t v0 = (int64_t)b * s.cap;
    __shared__ double part[2][kThreads];
    __shared__ int accepted;
    double tn = 0.0, tl = 0.0;
    for (int h = tid; h < s.cap; h += kThreads) {
        const int flag = s.dflag[v0 + h];
        if (flag == 0) continue;
        const double gn = fmin(s.g[v0 + h], g_max), gl = fmin(last_g[v0 + h], g_max);
        tn += flag == 1 ? log(gn) : log(1.0 - gn);
        tl += flag == 1 ? log(gl) : log(1.0 - gl);
    }
    part[0][tid] = tn;
    part[1][tid] = tl;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            part[0][tid] += part[0][tid + off];
            part[1][tid] += part[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double ln = l_new[b], ll = l_last[b], tp_new = part[0][0], tp_last = part[1][0];
        const double a = tempered ? exp((ln - ll) * beta[b] - tp_last + tp_new) : exp(ln - tp_last - ll + tp_new);
        accepted = u[b] < a;
        out[b * 4 + 0] = accepted;
        out[b * 4 + 1] = ln;
        out[b * 4 + 2] = tp_new;
        out[b * 4 + 3] = tp_last;
        if (accepted) l_last[b] = ln;
    }
    __syncthreads();
    if (!accepted) return;
    for (int h = tid; h < s.cap; h += kThreads) {
        last_feat[v0 + h] = s.feat[v0 + h];
        last_g[v0 + h] = s.g[v0 + h];
        last_lml[v0 + h] = lml[v0 + h];
        last_lcm[v0 + h] = lcm[v0 + h];
    }
    const int64_t nt = (int64_t)s.cap * (s.C + 1), np = (int64_t)s.cap * s.n_post;
    for (int64_t j = tid; j < nt; j += kThreads) last_thr[v0 * (s.C + 1) + j] = s.thr[v0 * (s.C + 1) + j];
    for (int64_t j = tid; j < np; j += kThreads) last_post[v0 * s.n_post + j] = s.post[v0 * s.n_post + j];
}

}  // namespace mtgrow
