// Kernels of include/mtree.h: the route pass, the segmented reduction of y, the one-launch bottom-up sweep and the
// predictive fold of a forest of meta-trees.
//
// (a) route_kernel<TC, TK>: one thread per (row, tree); blockIdx.y is the tree, so a wave walks one tree and its node reads
//     stay in a few cache lines near the root.  The rows' features are read where they lie; adjacent lanes read adjacent rows.
// (b) reduce_kernel<LDSH> / reduce_centred_kernel<LDSH>: a workgroup is ONE wave and owns a contiguous slab of rows of one tree
//     and a table only it writes (LDS when the tree's table fits MTREE_LDS_SLOTS, else its slab of global scratch, zeroed
//     by the caller).  Integer columns are integer atomics.  For a real column the wave takes 64 rows at a time; while lanes
//     remain, the first remaining lane's node id is broadcast, the lanes that share it are balloted, their addends (0.0 in
//     every other lane, which is exact) go through one xor butterfly, whose order is fixed by the lane numbers, and the
//     first lane of the group adds the result into the table.  combine_kernel adds the slabs in slab order.
// (c) sweep_kernel: a workgroup per tree, depth by depth from the deepest, a barrier in between; no waits across workgroups.
// (d) values_kernel (per node) and predict_kernel<TC, TK> (per row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtree.h"

namespace mtree {

constexpr int kThreads = 256;
constexpr int kWave = 64;

struct Forest {        // mtree_forest by value
    int n_trees, n_nodes, n_thr, max_depth, dim_cont, dim_cat;
    const int32_t *tree_off, *feat, *child0, *nchild, *thr_off, *depth;
    const double* thr;
};

__device__ __attribute__((noinline)) double lgamma_call(double x) { return lgamma(x); }

// The child of node v (table index) that row i goes to, or -1 where the walk stops.  [lo, hi) is the tree's node range.
template <typename TC, typename TK>
__device__ inline int next_node(const Forest& f, int v, int lo, int hi, const TC* __restrict__ xc, const TK* __restrict__ xk,
                                int64_t i) {
    const int ft = f.feat[v], nc = f.nchild[v];
    if (ft < 0 || nc < 1 || nc > MTREE_MAX_CHILDREN || ft >= f.dim_cont + f.dim_cat) return -1;
    int child = -1;
    if (ft < f.dim_cont) {
        const int to = f.thr_off[v];
        if (to < 0 || to + nc - 1 >= f.n_thr || !f.thr) return -1;       // reads thr[to + 1 .. to + nc - 1]
        const double x = (double)xc[i * f.dim_cont + ft];
        if (x < f.thr[to + 1]) child = 0;
        else if (f.thr[to + nc - 1] <= x) child = nc - 1;
        else
            for (int j = 1; j + 1 < nc; ++j)
                if (f.thr[to + j] <= x && x < f.thr[to + j + 1]) {
                    child = j;
                    break;
                }
    } else {
        const int64_t a = (int64_t)xk[i * f.dim_cat + (ft - f.dim_cont)];
        if ((uint64_t)a < (uint64_t)nc) child = (int)a;
    }
    if (child < 0) return -1;
    const int nx = f.child0[v] + child;
    return (nx > v && nx >= lo && nx < hi) ? nx : -1;
}

// ---- (a) ------------------------------------------------------------------------------------------------------------------
template <typename TC, typename TK>
__global__ __launch_bounds__(kThreads) void route_kernel(Forest f, const TC* __restrict__ xc, const TK* __restrict__ xk,
                                                         const int32_t* __restrict__ cat_card, int64_t n,
                                                         int32_t* __restrict__ stop, int32_t* __restrict__ path,
                                                         unsigned long long* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (b == 0) {      // the sample check, once per row
        long long nb = 0;
        if (i < n)
            for (int j = 0; j < f.dim_cat; ++j) nb += !((uint64_t)(int64_t)xk[i * f.dim_cat + j] < (uint64_t)cat_card[j]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nb += __shfl_down(nb, off);
        if ((threadIdx.x & 63) == 0 && nb > 0) atomicAdd(bad, (unsigned long long)nb);
    }
    if (i >= n) return;
    const int lo = f.tree_off[b], hi = f.tree_off[b + 1];
    if (lo < 0 || hi > f.n_nodes || lo >= hi) {
        stop[(int64_t)b * n + i] = -1;
        return;
    }
    int32_t* p = path ? path + ((int64_t)b * n + i) * (f.max_depth + 1) : nullptr;
    int v = lo, d = 0;
    for (;;) {
        if (p && d <= f.max_depth) p[d] = v;
        const int nx = d < MTREE_MAX_DEPTH ? next_node<TC, TK>(f, v, lo, hi, xc, xk, i) : -1;
        if (nx < 0) break;
        v = nx;
        ++d;
    }
    if (p)
        for (int j = d + 1; j <= f.max_depth; ++j) p[j] = -1;
    stop[(int64_t)b * n + i] = v;
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
// table[key] += the sum of `val` over the lanes whose key equals it, for every distinct key of the wave's active lanes.
// The add is a plain read-modify-write by the group's first lane, and the same entry may be written by another lane of this
// wave in a later round or a later 64 rows.  In LDS a wave's accesses are in order.  On the global-scratch path this relies
// on the memory operations of ONE wave to one address staying ordered (no other wave ever touches this wave's slab, so no
// fence or atomic is needed); tests/test_gpu_metatree.py::test_lds_and_global_tables holds that path to the exact oracle.
__device__ inline void wave_group_add(double* table, int stride, int key, bool active, double val) {
    unsigned long long rest = __ballot(active);
    const int lane = threadIdx.x & 63;
    while (rest) {
        const int lead = __ffsll((long long)rest) - 1;
        const int k0 = __shfl(key, lead);
        const unsigned long long same = __ballot(active && key == k0);
        double s = (active && key == k0) ? val : 0.0;
        if (__popcll(same) > 1) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        }
        if (lane == lead) table[(int64_t)k0 * stride] += s;
        rest &= ~same;
    }
}

// The same rounds for two columns of one entry (table[key * stride] += a, table[key * stride + 1] += b).
__device__ inline void wave_group_add2(double* table, int stride, int key, bool active, double a, double b) {
    unsigned long long rest = __ballot(active);
    const int lane = threadIdx.x & 63;
    while (rest) {
        const int lead = __ffsll((long long)rest) - 1;
        const int k0 = __shfl(key, lead);
        const bool in = active && key == k0;
        const unsigned long long same = __ballot(in);
        double s = in ? a : 0.0, q = in ? b : 0.0;
        if (__popcll(same) > 1) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                s += __shfl_xor(s, off);
                q += __shfl_xor(q, off);
            }
        }
        if (lane == lead) {
            table[(int64_t)k0 * stride] += s;
            table[(int64_t)k0 * stride + 1] += q;
        }
        rest &= ~same;
    }
}

struct Slab {
    int64_t lo, hi;
};
__device__ inline Slab slab_of(int64_t n, int S, int s) {
    int64_t span = (n + S - 1) / S;
    span = (span + kWave - 1) / kWave * kWave;
    Slab r;
    r.lo = (int64_t)s * span;
    r.hi = r.lo + span < n ? r.lo + span : n;
    return r;
}

// grid (S, n_trees), 64 threads.  work_int: [S][n_nodes][ni], work_real: [S][n_nodes][nr1] (nr1 = real columns of this pass).
template <bool LDSH>
__global__ __launch_bounds__(kWave) void reduce_kernel(Forest f, int family, int degree, int ni, int nr1,
                                                       const int32_t* __restrict__ stop, const void* __restrict__ y,
                                                       const double* __restrict__ pivot, int64_t n, int S,
                                                       unsigned long long* __restrict__ work_int,
                                                       double* __restrict__ work_real) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int b = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
    const int t0 = f.tree_off[b], nn = f.tree_off[b + 1] - t0;
    if (t0 < 0 || nn < 1 || t0 + nn > f.n_nodes) return;
    unsigned long long* gi = work_int + ((int64_t)s * f.n_nodes + t0) * ni;
    double* gr = work_real + ((int64_t)s * f.n_nodes + t0) * nr1;
    unsigned long long* ti = LDSH ? (unsigned long long*)lds : gi;
    double* tr = LDSH ? (double*)(lds + sizeof(unsigned long long) * (size_t)nn * ni) : gr;
    if (LDSH) {
        for (int j = lane; j < nn * ni; j += kWave) ti[j] = 0ull;
        for (int j = lane; j < nn * nr1; j += kWave) tr[j] = 0.0;
        __syncthreads();
    }
    const Slab sl = slab_of(n, S, s);
    // (pivot: a value taken off every y of normal before it is summed; mtree_reduce passes none)
    const double pv = (family == MTREE_NORMAL && pivot) ? pivot[0] : 0.0;
    const bool discrete = family <= MTREE_POISSON;
    for (int64_t base = sl.lo; base < sl.hi; base += kWave) {
        const int64_t i = base + lane;
        bool active = i < sl.hi;
        int key = active ? stop[(int64_t)b * n + i] - t0 : -1;
        active = active && key >= 0 && key < nn;
        double rv = 0.0;
        if (active) {
            atomicAdd(&ti[(int64_t)key * ni], 1ull);
            if (discrete) {
                const int64_t v = ((const int64_t*)y)[i];
                if (family == MTREE_BERNOULLI) {
                    if (v == 1) atomicAdd(&ti[(int64_t)key * ni + 1], 1ull);
                } else if (family == MTREE_CATEGORICAL) {
                    if ((uint64_t)v < (uint64_t)degree) atomicAdd(&ti[(int64_t)key * ni + 1 + v], 1ull);
                } else if (v >= 0) {
                    atomicAdd(&ti[(int64_t)key * ni + 1], (unsigned long long)v);
                    rv = lgamma_call((double)v + 1.0);
                }
            } else {
                rv = ((const double*)y)[i] - pv;
            }
        }
        if (nr1 > 0) wave_group_add(tr, nr1, key, active, rv);
    }
    if (LDSH) {
        __syncthreads();
        for (int j = lane; j < nn * ni; j += kWave) gi[j] = ti[j];
        for (int j = lane; j < nn * nr1; j += kWave) gr[j] = tr[j];
    }
}

// The second pass of normal.  mu = stat_real[node][0] / stat_int[node][0] of the combined first pass is the stop node's own
// expansion point: the pass sums r = y - mu and r^2 (work_real: [S][n_nodes][2]).  The node's mean is mu + (sum r) / n, so
// what the plain sum of the first pass lost comes back in sum r, and no row is ever measured from another node's level.
template <bool LDSH>
__global__ __launch_bounds__(kWave) void reduce_centred_kernel(Forest f, const int32_t* __restrict__ stop,
                                                               const double* __restrict__ y, int64_t n, int S,
                                                               const int64_t* __restrict__ stat_int,
                                                               const double* __restrict__ stat_real, int nr,
                                                               double* __restrict__ work_real) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int b = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
    const int t0 = f.tree_off[b], nn = f.tree_off[b + 1] - t0;
    if (t0 < 0 || nn < 1 || nn > MTREE_MAX_NODES || t0 + nn > f.n_nodes) return;
    double* gr = work_real + ((int64_t)s * f.n_nodes + t0) * 2;
    double* tr = LDSH ? (double*)lds : gr;
    if (LDSH) {
        for (int j = lane; j < nn * 2; j += kWave) tr[j] = 0.0;
        __syncthreads();
    }
    const Slab sl = slab_of(n, S, s);
    for (int64_t base = sl.lo; base < sl.hi; base += kWave) {
        const int64_t i = base + lane;
        bool active = i < sl.hi;
        int key = active ? stop[(int64_t)b * n + i] - t0 : -1;
        active = active && key >= 0 && key < nn;
        double r = 0.0;
        if (active) {
            const int64_t cnt = stat_int[t0 + key];
            const double mu = cnt > 0 ? stat_real[(int64_t)(t0 + key) * nr] / (double)cnt : 0.0;
            r = y[i] - mu;
        }
        wave_group_add2(tr, 2, key, active, r, r * r);
    }
    if (LDSH) {
        __syncthreads();
        for (int j = lane; j < nn * 2; j += kWave) gr[j] = tr[j];
    }
}

// out[node * out_stride + out_col + c] = sum over slabs, in slab order, of work[(s * n_nodes + node) * cols + c].
template <typename T>
__global__ __launch_bounds__(kThreads) void combine_kernel(const T* __restrict__ work, int S, int64_t n_nodes, int cols,
                                                           int out_stride, int out_col, T* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n_nodes * cols) return;
    const int64_t node = j / cols;
    const int c = (int)(j - node * cols);
    T acc = 0;
    for (int s = 0; s < S; ++s) acc += work[((int64_t)s * n_nodes + node) * cols + c];
    out[node * out_stride + out_col + c] = acc;
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
// Children's totals into node v's (in place), then the fold and lml.  Returns false (nothing written) when n = 0.
__device__ inline bool fold_node(const Forest& f, int family, int degree, int ni, int nr, int np, int v, int lo, int hi,
                                 int64_t* __restrict__ si, double* __restrict__ sr, const double* __restrict__ h0,
                                 double* __restrict__ post, double* lml_out) {
    int64_t* ci = si + (int64_t)v * ni;
    double* cr = sr + (int64_t)v * nr;
    const int nc = f.feat[v] >= 0 ? f.nchild[v] : 0;
    const int c0 = f.child0[v];
    const bool kids = nc > 0 && nc <= MTREE_MAX_CHILDREN && c0 > v && c0 >= lo && c0 + nc <= hi;
    if (family == MTREE_NORMAL) {
        // A node's three columns are (mu, c, SS): its mean is mu + c / n and SS is about that mean.  The reduction left
        // (sum y, sum r, sum r^2) of the node's own rows, r = y - mu with mu = (sum y) / n: sum (r - c/n)^2 = sum r^2 - c^2/n.
        const int64_t n_own = ci[0];
        double mu = 0.0, c = 0.0, ss = 0.0;
        if (n_own > 0) {
            mu = cr[0] / (double)n_own;
            c = cr[1];
            ss = fmax(cr[2] - c * c / (double)n_own, 0.0);
        }
        int64_t n_tot = n_own;
        if (kids)
            for (int k = 0; k < nc; ++k) n_tot += si[(int64_t)(c0 + k) * ni];
        if (n_tot > n_own) {
            // The parts (own rows, children) merge about muP, the rounded mean of them all, so that every n (mu - muP) is
            // known to an ulp of sum |y|; cP takes what is left.  All dm use the same cP / n, whose error therefore enters
            // SS only squared.
            double w = n_own > 0 ? (double)n_own * (mu + c / (double)n_own) : 0.0;
            for (int k = 0; k < nc; ++k) {
                const int64_t n_c = si[(int64_t)(c0 + k) * ni];
                const double* kr = sr + (int64_t)(c0 + k) * nr;
                if (n_c > 0) w += (double)n_c * (kr[0] + kr[1] / (double)n_c);
            }
            const double muP = w / (double)n_tot;
            double cP = n_own > 0 ? c + (double)n_own * (mu - muP) : 0.0;
            for (int k = 0; k < nc; ++k) {
                const int64_t n_c = si[(int64_t)(c0 + k) * ni];
                const double* kr = sr + (int64_t)(c0 + k) * nr;
                if (n_c > 0) cP += kr[1] + (double)n_c * (kr[0] - muP);
            }
            const double off = cP / (double)n_tot;
            double ssP = 0.0;
            if (n_own > 0) {
                const double dm = (mu - muP) + (c / (double)n_own - off);
                ssP += ss + (double)n_own * dm * dm;
            }
            for (int k = 0; k < nc; ++k) {
                const int64_t n_c = si[(int64_t)(c0 + k) * ni];
                const double* kr = sr + (int64_t)(c0 + k) * nr;
                if (n_c > 0) {
                    const double dm = (kr[0] - muP) + (kr[1] / (double)n_c - off);
                    ssP += kr[2] + (double)n_c * dm * dm;
                }
            }
            mu = muP;
            c = cP;
            ss = ssP;
        }
        if (n_tot > 0) {
            cr[0] = mu;
            cr[1] = c;
            cr[2] = ss;
        }
        ci[0] = n_tot;
    } else if (kids) {
        for (int j = 0; j < ni; ++j) {
            int64_t t = ci[j];
            for (int c = 0; c < nc; ++c) t += si[(int64_t)(c0 + c) * ni + j];
            ci[j] = t;
        }
        for (int j = 0; j < nr; ++j) {
            double t = cr[j];
            for (int c = 0; c < nc; ++c) t += sr[(int64_t)(c0 + c) * nr + j];
            cr[j] = t;
        }
    }
    const int64_t n = ci[0];
    if (n <= 0) return false;
    double* p = post + (int64_t)v * np;
    double lml = 0.0;
    if (family == MTREE_BERNOULLI) {
        p[0] += (double)ci[1];
        p[1] += (double)(n - ci[1]);
        lml = lgamma_call(h0[0] + h0[1]) - lgamma_call(h0[0]) - lgamma_call(h0[1]) - lgamma_call(p[0] + p[1]) +
              lgamma_call(p[0]) + lgamma_call(p[1]);
    } else if (family == MTREE_CATEGORICAL) {
        double s0 = 0.0, l0 = 0.0, sn = 0.0, ln = 0.0;
        for (int a = 0; a < degree; ++a) {
            p[a] += (double)ci[1 + a];
            s0 += h0[a];
            l0 += lgamma_call(h0[a]);
            sn += p[a];
            ln += lgamma_call(p[a]);
        }
        lml = lgamma_call(s0) - l0 - lgamma_call(sn) + ln;
    } else if (family == MTREE_POISSON) {
        p[0] += (double)ci[1];
        p[1] += (double)n;
        p[2] += cr[0];
        lml = h0[0] * log(h0[1]) - lgamma_call(h0[0]) - p[0] * log(p[1]) + lgamma_call(p[0]) - p[2];
    } else if (family == MTREE_EXPONENTIAL) {
        p[0] += (double)n;
        p[1] += cr[0];
        lml = h0[0] * log(h0[1]) - lgamma_call(h0[0]) - p[0] * log(p[1]) + lgamma_call(p[0]);
    } else {
        // (the difference to the prior mean from mu, not from the rounded x_bar: m and mu may be close)
        const double dn = (double)n, off = cr[1] / dn, x_bar = cr[0] + off, dm = (cr[0] - p[0]) + off;
        p[3] += (cr[2] + dn * p[1] / (p[1] + dn) * (dm * dm)) / 2.0;
        p[0] = (p[1] * p[0] + dn * x_bar) / (p[1] + dn);
        p[1] += dn;
        p[2] += dn * 0.5;
        p[4] += dn;
        lml = h0[2] * log(h0[3]) - p[2] * log(p[3]) + lgamma_call(p[2]) - lgamma_call(h0[2]) +
              0.5 * (log(h0[1]) - log(p[1]) - p[4] * 1.8378770664093453);
    }
    *lml_out = lml;
    return true;
}

// grid n_trees, kThreads threads.  L: [n_nodes] scratch.
__global__ __launch_bounds__(kThreads) void sweep_kernel(Forest f, int family, int degree, int ni, int nr, int np,
                                                         int64_t* __restrict__ si, double* __restrict__ sr,
                                                         const double* __restrict__ h0, double* __restrict__ post, double* __restrict__ g,
                                                         double* __restrict__ lml, double* __restrict__ lcm,
                                                         double* __restrict__ lnp, double* __restrict__ L) {
    const int b = blockIdx.x;
    const int lo = f.tree_off[b], hi = f.tree_off[b + 1];
    if (lo < 0 || hi > f.n_nodes || lo >= hi) return;       // (uniform over the workgroup)
    for (int d = f.max_depth; d >= 0; --d) {
        for (int v = lo + threadIdx.x; v < hi; v += kThreads) {
            if (f.depth[v] != d) continue;
            double own = 0.0;
            if (!fold_node(f, family, degree, ni, nr, np, v, lo, hi, si, sr, h0, post, &own)) {
                L[v] = 0.0;
                continue;
            }
            lml[v] = own;
            const int nc = f.feat[v] >= 0 ? f.nchild[v] : 0;
            const int c0 = f.child0[v];
            double out = own;
            if (nc > 0 && nc <= MTREE_MAX_CHILDREN && c0 > v && c0 >= lo && c0 + nc <= hi) {
                double S = 0.0;
                for (int c = 0; c < nc; ++c) {
                    S += L[c0 + c];
                    lcm[c0 + c] = L[c0 + c];
                }
                const double g0 = g[v];
                if (!(g0 > 0.0)) {
                    out = own;
                    g[v] = 0.0;
                } else if (!(g0 < 1.0)) {
                    out = S;
                    g[v] = 1.0;
                } else {
                    const double A = log1p(-g0) + own, B = log(g0) + S;
                    const double t = A - B;
                    out = t == 0.0 ? A + 0.6931471805599453 : t > 0.0 ? A + log1p(exp(-t)) : B + log1p(exp(t));
                    // next to 1 (t < 0), B - out is known to an ulp of B only; 1 / (1 + e^t) keeps the digits of 1 - g
                    g[v] = t > 0.0 ? exp(B - out) : 1.0 / (1.0 + exp(t));
                }
            }
            L[v] = out;
            if (v == lo) lnp[b] += out;
        }
        __syncthreads();
    }
}

// ---- (d) ------------------------------------------------------------------------------------------------------------------
// V[node][C] (and for VAR the second table V2[node]) from the posteriors, in the scalar learners' order of operations.
__global__ __launch_bounds__(kThreads) void values_kernel(int n_nodes, int family, int degree, int mode, int np, int C,
                                                          const double* __restrict__ post, double* __restrict__ V) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n_nodes) return;
    const double* p = post + (int64_t)v * np;
    double* o = V + (int64_t)v * C;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (family == MTREE_BERNOULLI) {
        const double th = p[0] / (p[0] + p[1]);
        o[0] = 1.0 - th;
        o[1] = th;
    } else if (family == MTREE_CATEGORICAL) {
        double s = 0.0;
        for (int a = 0; a < degree; ++a) s += p[a];
        for (int a = 0; a < degree; ++a) o[a] = p[a] / s;
    } else if (family == MTREE_POISSON) {
        const double th = 1.0 / (1.0 + p[1]);
        o[0] = p[0] * th / (1.0 - th);
    } else if (family == MTREE_EXPONENTIAL) {
        o[0] = p[0] > 1.0 ? p[1] / (p[0] - 1.0) : nan;
    } else {
        o[0] = p[0];
        if (mode == MTREE_PRED_VAR) {
            const double nu = 2.0 * p[2], lam = p[1] / (p[1] + 1.0) * p[2] / p[3];
            V[(int64_t)n_nodes + v] = nu > 2.0 ? nu / lam / (nu - 2.0) : nan;
        }
    }
}

// One thread per row.  The walk's nodes are kept (at most MTREE_MAX_DEPTH + 1) and folded from the stop node up.
template <typename TC, typename TK>
__global__ __launch_bounds__(kThreads) void predict_kernel(Forest f, int mode, int C, const TC* __restrict__ xc,
                                                           const TK* __restrict__ xk, int64_t n,
                                                           const double* __restrict__ g, const double* __restrict__ prob,
                                                           const double* __restrict__ V, void* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int nodes[MTREE_MAX_DEPTH + 1];
    double acc[MTREE_MAX_DEGREE], val[MTREE_MAX_DEGREE];
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    const double* V2 = V + f.n_nodes;
    double mix_mean = 0.0, var_acc = 0.0;
    const int passes = mode == MTREE_PRED_VAR ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        for (int b = 0; b < f.n_trees; ++b) {
            const int lo = f.tree_off[b], hi = f.tree_off[b + 1];
            if (lo < 0 || hi > f.n_nodes || lo >= hi) continue;
            int d = 0;
            nodes[0] = lo;
            while (d < MTREE_MAX_DEPTH) {
                const int nx = next_node<TC, TK>(f, nodes[d], lo, hi, xc, xk, i);
                if (nx < 0) break;
                nodes[++d] = nx;
            }
            const double pb = prob[b];
            if (mode == MTREE_PRED_VAR) {
                double m = V[nodes[d]], s2 = V2[nodes[d]];
                for (int j = d - 1; j >= 0; --j) {
                    const int v = nodes[j];
                    const double gv = g[v], mv = V[v], vv = V2[v];
                    const double mm = (1.0 - gv) * mv + gv * m;
                    s2 = (1.0 - gv) * ((mm - mv) * (mm - mv) + vv) + gv * ((mm - m) * (mm - m) + s2);
                    m = mm;
                }
                if (pass == 0) mix_mean += pb * m;
                else var_acc += pb * ((m - mix_mean) * (m - mix_mean) + s2);
            } else {
                for (int c = 0; c < C; ++c) val[c] = V[(int64_t)nodes[d] * C + c];
                for (int j = d - 1; j >= 0; --j) {
                    const int v = nodes[j];
                    const double gv = g[v];
                    for (int c = 0; c < C; ++c) val[c] = (1.0 - gv) * V[(int64_t)v * C + c] + gv * val[c];
                }
                for (int c = 0; c < C; ++c) acc[c] += pb * val[c];
            }
        }
    }
    if (mode == MTREE_PRED_VAR) ((double*)out)[i] = var_acc;
    else if (mode == MTREE_PRED_CLASS) {
        int best = 0;
        for (int c = 1; c < C; ++c)
            if (acc[c] > acc[best]) best = c;
        ((int64_t*)out)[i] = best;
    } else
        for (int c = 0; c < C; ++c) ((double*)out)[i * C + c] = acc[c];
}

}  // namespace mtree
