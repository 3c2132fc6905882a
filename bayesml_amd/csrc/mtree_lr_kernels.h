// Kernels of include/mtree.h for MTREE_LINREG: every node carries a Bayesian linear regression over all continuous
// features (degree D <= MTREE_LR_MAX_DEGREE), so a node's statistics are X'X, X'y, y'y and n of its rows.
//
// (e) Order.  lr_hist_kernel counts, per row slab and per stop node, the rows of a tree (integer atomics: exact and
//     order-free); lr_scan_kernel turns the counts into positions, node-major and slab-minor, and leaves every node's n and
//     the start of its segment; lr_scatter_kernel lets one wave per (slab, tree) write its rows in row order.  The result is
//     the tree's row indices sorted stably by (stop node, row index): no position depends on the order atomics land in.
// (f) lr_gram_kernel<TC>: one wave per block of MTREE_LR_BLOCK sorted positions.  The augmented row z = [x_0..x_{D-1}, y]
//     padded with zeros to 16 is both operands of v_mfma_f64_16x16x4_f64 (lane l supplies z_{row l>>4}[l&15]), so one
//     instruction adds four rows' z z' to the wave's one accumulator tile Z'Z.  The wave walks its block run by run (a run =
//     the positions of one node); rows past a run's end inside a quad are zero rows, which is exact.  A run that lies
//     strictly inside the block is the node's whole segment and goes to the node's statistics; the block's first and last
//     run go to the block's two boundary slots, and lr_fixup_kernel adds the slots of a node in block order.  No
//     floating-point atomics anywhere: the sums' order is fixed by the sorted order and the block length alone.
// (g) lr_prior_kernel (ln|Lambda_h0|, once per call) and lr_sweep_kernel, sweep_kernel's sibling: a workgroup per tree, a
//     barrier per depth, no waits across workgroups.
// (h) lr_values_kernel (per node: mu, the packed inverse Cholesky factor of Lambda, alpha / beta, 2 alpha) and
//     lr_predict_kernel<TC, TK> (per row).
#pragma once
#include "common.h"
#include "mtree_kernels.h"

namespace mtree {
using gmmvb::d4;
using gmmvb::mfma_f64;

constexpr int kLrD = MTREE_LR_MAX_DEGREE;
constexpr int kLrTri = kLrD * (kLrD + 1) / 2;
constexpr int kLrQuads = 8;       // quads (of four rows) whose loads a lane has in flight before the first MFMA
constexpr double kLn2Pi = 1.8378770664093453;

__host__ __device__ inline int lr_tri(int D) { return D * (D + 1) / 2; }
// index of (i, j), i <= j, in the row-major upper triangle of a D x D matrix
__device__ inline int lr_ut(int D, int i, int j) { return i * D - i * (i - 1) / 2 + (j - i); }
// the same entry of the symmetric matrix for any (i, j)
__device__ inline int lr_sym(int D, int i, int j) { return i <= j ? lr_ut(D, i, j) : lr_ut(D, j, i); }
// index of (i, j), j <= i, in a row-major packed lower triangle
__device__ inline int lr_lt(int i, int j) { return i * (i + 1) / 2 + j; }

// ---- (e) ------------------------------------------------------------------------------------------------------------------
// grid (S, n_trees), kThreads threads.  hist: [S][n_nodes] int32; the workgroup counts its slab in LDS and writes every
// entry of its tree's row, so the table needs no zeroing.
__global__ __launch_bounds__(kThreads) void lr_hist_kernel(Forest f, const int32_t* __restrict__ stop, int64_t n, int S,
                                                           int32_t* __restrict__ hist) {
    __shared__ int cnt[MTREE_MAX_NODES];
    const int b = blockIdx.y, s = blockIdx.x;
    const int t0 = f.tree_off[b], nn = f.tree_off[b + 1] - t0;
    if (t0 < 0 || nn < 1 || nn > MTREE_MAX_NODES || t0 + nn > f.n_nodes) return;      // (uniform over the workgroup)
    for (int j = threadIdx.x; j < nn; j += kThreads) cnt[j] = 0;
    __syncthreads();
    const Slab sl = slab_of(n, S, s);
    for (int64_t i = sl.lo + threadIdx.x; i < sl.hi; i += kThreads) {
        const int key = stop[(int64_t)b * n + i] - t0;
        if (key >= 0 && key < nn) atomicAdd(&cnt[key], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nn; j += kThreads) hist[(int64_t)s * f.n_nodes + t0 + j] = cnt[j];
}

// grid n_trees, kThreads threads.  In place: hist[s][v] becomes the position (in the tree's sorted array) of the first row
// of slab s that stops at v.  start[v] = the position of v's segment, stat_int[v * ni] = its length, tree_cnt[b] = the
// tree's rows that stop at one of its nodes.
__global__ __launch_bounds__(kThreads) void lr_scan_kernel(Forest f, int S, int ni, int32_t* __restrict__ hist,
                                                           int32_t* __restrict__ start, int64_t* __restrict__ stat_int,
                                                           int32_t* __restrict__ tree_cnt) {
    __shared__ int part[kThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const int t0 = f.tree_off[b], nn = f.tree_off[b + 1] - t0;
    if (t0 < 0 || nn < 1 || nn > MTREE_MAX_NODES || t0 + nn > f.n_nodes) {      // (uniform over the workgroup)
        if (t == 0) tree_cnt[b] = 0;
        return;
    }
    const int chunk = (nn + kThreads - 1) / kThreads;
    const int v0 = t * chunk < nn ? t * chunk : nn, v1 = v0 + chunk < nn ? v0 + chunk : nn;
    int mine = 0;
    for (int v = v0; v < v1; ++v)
        for (int s = 0; s < S; ++s) mine += hist[(int64_t)s * f.n_nodes + t0 + v];
    part[t] = mine;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int j = 0; j < kThreads; ++j) {
            const int c = part[j];
            part[j] = run;
            run += c;
        }
        tree_cnt[b] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int v = v0; v < v1; ++v) {
        start[t0 + v] = run;
        int c = 0;
        for (int s = 0; s < S; ++s) {
            int32_t* h = hist + (int64_t)s * f.n_nodes + t0 + v;
            const int k = *h;
            *h = run + c;
            c += k;
        }
        stat_int[(int64_t)(t0 + v) * ni] = c;
        run += c;
    }
}

// grid (S, n_trees), ONE wave.  The wave owns its slab's counters (a copy in LDS) and takes 64 consecutive rows at a time:
// a row's position is its node's counter plus the number of lower lanes with the same node, so the slab's rows of a node
// keep their row order; the highest lane of a node then advances the counter.
__global__ __launch_bounds__(kWave) void lr_scatter_kernel(Forest f, const int32_t* __restrict__ stop, int64_t n, int S,
                                                           const int32_t* __restrict__ off, int32_t* __restrict__ sorted) {
    __shared__ int cnt[MTREE_MAX_NODES];
    const int b = blockIdx.y, s = blockIdx.x, lane = threadIdx.x;
    const int t0 = f.tree_off[b], nn = f.tree_off[b + 1] - t0;
    if (t0 < 0 || nn < 1 || nn > MTREE_MAX_NODES || t0 + nn > f.n_nodes) return;
    for (int j = lane; j < nn; j += kWave) cnt[j] = off[(int64_t)s * f.n_nodes + t0 + j];
    __syncthreads();
    const Slab sl = slab_of(n, S, s);
    for (int64_t base = sl.lo; base < sl.hi; base += kWave) {
        const int64_t i = base + lane;
        int key = i < sl.hi ? stop[(int64_t)b * n + i] - t0 : -1;
        if (key < 0 || key >= nn) key = -1;
        int below = 0, above = 0;
        for (int j = 0; j < kWave; ++j) {
            const int kj = __shfl(key, j);
            below += (kj == key && j < lane);
            above += (kj == key && j > lane);
        }
        const int pos = key >= 0 ? cnt[key] + below : -1;
        __syncthreads();
        if (key >= 0) {
            if (pos >= 0 && pos < n) sorted[(int64_t)b * n + pos] = (int32_t)i;
            if (above == 0) cnt[key] = pos + 1;
        }
        __syncthreads();
    }
}

// ---- (f) ------------------------------------------------------------------------------------------------------------------
// The node of tree [t0, t0 + nn) whose segment holds position p (p < the tree's count): the last v with start[v] <= p.  Empty
// nodes share their start with the next node, so the last one is the non-empty one.
__device__ inline int lr_node_at(const int32_t* __restrict__ start, int t0, int nn, int p) {
    int lo = 0, hi = nn - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[t0 + mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The statistics of a finished accumulator tile: lane l holds C[(l>>4) + 4 r][l&15] in element r.
__device__ inline void lr_store_tile(const d4& acc, int D, int lane, double* __restrict__ dst) {
    const int j = lane & 15, T = lr_tri(D);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = (lane >> 4) + 4 * r;
        if (i <= j && j < D) dst[lr_ut(D, i, j)] = acc[r];
        else if (i < D && j == D) dst[T + i] = acc[r];
        else if (i == D && j == D) dst[T + D] = acc[r];
    }
}

// grid (blocks of the longest tree, n_trees), ONE wave.  x: rows of `stride` elements of TC; y: binary64.  slot_key:
// [n_trees][nblk][2] (node, or -1 for an unused slot), slot_val: [n_trees][nblk][2][nr].
template <typename TC>
__global__ __launch_bounds__(kWave) void lr_gram_kernel(Forest f, int D, const TC* __restrict__ x, int64_t stride,
                                                        const double* __restrict__ y, int64_t n,
                                                        const int32_t* __restrict__ sorted,
                                                        const int32_t* __restrict__ start,
                                                        const int64_t* __restrict__ stat_int, int ni,
                                                        const int32_t* __restrict__ tree_cnt, int nr,
                                                        double* __restrict__ stat_real, int32_t* __restrict__ slot_key,
                                                        double* __restrict__ slot_val) {
    const int b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x, lane = threadIdx.x;
    const int64_t slot0 = ((int64_t)b * nblk + blk) * 2;
    const int t0 = f.tree_off[b], nn = f.tree_off[b + 1] - t0;
    int cnt = (t0 < 0 || nn < 1 || nn > MTREE_MAX_NODES || t0 + nn > f.n_nodes) ? 0 : tree_cnt[b];
    if (cnt > n) cnt = (int)n;
    const int64_t p0 = (int64_t)blk * MTREE_LR_BLOCK;
    if (p0 >= cnt) {
        if (lane < 2) slot_key[slot0 + lane] = -1;
        return;
    }
    const int pend = (int)(p0 + MTREE_LR_BLOCK < cnt ? p0 + MTREE_LR_BLOCK : cnt);
    const int32_t* idx = sorted + (int64_t)b * n;
    const int e = lane & 15, r = lane >> 4;
    bool last_used = false;
    int p = (int)p0;
    while (p < pend) {
        const int v = lr_node_at(start, t0, nn, p);
        const int64_t seg = start[t0 + v] + stat_int[(int64_t)(t0 + v) * ni];
        int q1 = seg < pend ? (int)seg : pend;
        if (q1 <= p) q1 = pend;            // (a malformed table: the rest of the block is one run, never an endless loop)
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int q = p; q < q1; q += 4 * kLrQuads) {
            int64_t row[kLrQuads];
            double z[kLrQuads];
#pragma unroll
            for (int u = 0; u < kLrQuads; ++u) {
                const int pos = q + 4 * u + r;
                row[u] = pos < q1 ? (int64_t)idx[pos] : -1;
            }
#pragma unroll
            for (int u = 0; u < kLrQuads; ++u) {
                const bool ok = row[u] >= 0 && row[u] < n;
                z[u] = !ok ? 0.0 : e < D ? (double)x[row[u] * stride + e] : e == D ? y[row[u]] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kLrQuads; ++u) acc = mfma_f64(z[u], z[u], acc);
        }
        const bool first = p == (int)p0, last = q1 == pend;
        if (first || last) {
            const int which = first ? 0 : 1;
            if (lane == 0) slot_key[slot0 + which] = t0 + v;
            lr_store_tile(acc, D, lane, slot_val + (slot0 + which) * nr);
            last_used = last_used || !first;
        } else {
            lr_store_tile(acc, D, lane, stat_real + (int64_t)(t0 + v) * nr);
        }
        p = q1;
    }
    if (!last_used && lane == 0) slot_key[slot0 + 1] = -1;
}

// grid (2 nblk, n_trees), ONE wave per boundary slot.  The slots of a tree in block order hold every node's pieces next to
// each other (-1 = unused).  The wave of a node's first slot adds the node's slots in that order, a lane per column.
__global__ __launch_bounds__(kWave) void lr_fixup_kernel(int n_nodes, int nr, const int32_t* __restrict__ slot_key,
                                                         const double* __restrict__ slot_val,
                                                         double* __restrict__ stat_real) {
    const int b = blockIdx.y, j = blockIdx.x, ns = gridDim.x;
    const int32_t* key = slot_key + (int64_t)b * ns;
    const int k = key[j];
    if (k < 0 || k >= n_nodes) return;
    int before = -1;
    for (int i = j - 1; i >= 0 && before < 0; --i) before = key[i];
    if (before == k) return;
    for (int c = threadIdx.x; c < nr; c += kWave) {
        double acc = 0.0;
        for (int i = j; i < ns; ++i) {
            const int ki = key[i];
            if (ki < 0) continue;
            if (ki != k) break;
            acc += slot_val[((int64_t)b * ns + i) * nr + c];
        }
        stat_real[(int64_t)k * nr + c] = acc;
    }
}

// ---- (g) ------------------------------------------------------------------------------------------------------------------
// In place: the packed upper triangle A of a symmetric positive definite matrix becomes U with A = U'U (U upper, so
// L = U').  Returns ln|A|.  A matrix that is not positive definite gives NaN, never a bad index.
__device__ inline double lr_cholesky(double* A, int D) {
    double lndet = 0.0;
    for (int i = 0; i < D; ++i) {
        double d = A[lr_ut(D, i, i)];
        for (int k = 0; k < i; ++k) d -= A[lr_ut(D, k, i)] * A[lr_ut(D, k, i)];
        d = sqrt(d);
        A[lr_ut(D, i, i)] = d;
        lndet += log(d);
        for (int j = i + 1; j < D; ++j) {
            double s = A[lr_ut(D, i, j)];
            for (int k = 0; k < i; ++k) s -= A[lr_ut(D, k, i)] * A[lr_ut(D, k, j)];
            A[lr_ut(D, i, j)] = s / d;
        }
    }
    return 2.0 * lndet;
}

// One thread: out[0] = ln|Lambda_h0| of the prior vector h0 = [mu | upper triangle of Lambda | a | b | 0].
__global__ void lr_prior_kernel(int D, const double* __restrict__ h0, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0 || D < 1 || D > kLrD) return;
    double A[kLrTri];
    const int T = lr_tri(D);
    for (int k = 0; k < T; ++k) A[k] = h0[D + k];
    out[0] = lr_cholesky(A, D);
}

// Children's totals into node v's (in place, child order), then the fold onto the node's current posterior
//   Lambda = Lambda0 + X'X,  mu = Lambda^-1 c with c = X'y + Lambda0 mu0,  alpha = alpha0 + n / 2,
//   beta = beta0 + (y'y + mu0'Lambda0 mu0 - |w|^2) / 2 with w = L^-1 c (so that |w|^2 = mu'Lambda mu),  n_cum = n0 + n
// and lml against the prior (a, b, ln|Lambda_h0|).  Returns false (nothing written) when no row passes v.
__device__ inline bool lr_fold_node(const Forest& f, int D, int ni, int nr, int np, int v, int lo, int hi,
                                    int64_t* __restrict__ si, double* __restrict__ sr, const double* __restrict__ h0,
                                    double lndet0, double* __restrict__ post, double* lml_out) {
    const int T = lr_tri(D);
    int64_t* ci = si + (int64_t)v * ni;
    double* cr = sr + (int64_t)v * nr;
    const int nc = f.feat[v] >= 0 ? f.nchild[v] : 0;
    const int c0 = f.child0[v];
    if (nc > 0 && nc <= MTREE_MAX_CHILDREN && c0 > v && c0 >= lo && c0 + nc <= hi) {
        int64_t t = ci[0];
        for (int c = 0; c < nc; ++c) t += si[(int64_t)(c0 + c) * ni];
        ci[0] = t;
        for (int j = 0; j < nr; ++j) {
            double a = cr[j];
            for (int c = 0; c < nc; ++c) a += sr[(int64_t)(c0 + c) * nr + j];
            cr[j] = a;
        }
    }
    const int64_t n = ci[0];
    if (n <= 0) return false;
    double* p = post + (int64_t)v * np;
    double A[kLrTri], w[kLrD];
    // c = X'y + Lambda0 mu0 and mu0'Lambda0 mu0, from the posterior the fold starts from
    double m0 = 0.0;
    for (int i = 0; i < D; ++i) {
        double t = 0.0;
        for (int j = 0; j < D; ++j) t += p[D + lr_sym(D, i, j)] * p[j];
        m0 += p[i] * t;
        w[i] = cr[T + i] + t;
    }
    for (int k = 0; k < T; ++k) {
        A[k] = p[D + k] + cr[k];
        p[D + k] = A[k];
    }
    const double lndet = lr_cholesky(A, D);
    double ww = 0.0;
    for (int i = 0; i < D; ++i) {             // w = U'^-1 c
        double t = w[i];
        for (int k = 0; k < i; ++k) t -= A[lr_ut(D, k, i)] * w[k];
        w[i] = t / A[lr_ut(D, i, i)];
        ww += w[i] * w[i];
    }
    const double dn = (double)n;
    p[D + T] += dn * 0.5;
    p[D + T + 1] += 0.5 * (cr[T + D] + m0 - ww);
    p[D + T + 2] += dn;
    for (int i = D - 1; i >= 0; --i) {        // mu = U^-1 w
        double t = w[i];
        for (int k = i + 1; k < D; ++k) t -= A[lr_ut(D, i, k)] * w[k];
        w[i] = t / A[lr_ut(D, i, i)];
        p[i] = w[i];
    }
    const double a0 = h0[D + T], b0 = h0[D + T + 1], al = p[D + T], be = p[D + T + 1];
    *lml_out = a0 * log(b0) - al * log(be) + lgamma_call(al) - lgamma_call(a0) +
               0.5 * (lndet0 - lndet - p[D + T + 2] * kLn2Pi);
    return true;
}

// sweep_kernel's two-way mixture of an inner node: returns L and updates g[v] (0 and 1 are fixed points).
__device__ inline double lr_mix(double* __restrict__ g, int v, double own, double S) {
    const double g0 = g[v];
    if (!(g0 > 0.0)) {
        g[v] = 0.0;
        return own;
    }
    if (!(g0 < 1.0)) {
        g[v] = 1.0;
        return S;
    }
    const double A = log1p(-g0) + own, B = log(g0) + S;
    const double t = A - B;
    const double out = t == 0.0 ? A + 0.6931471805599453 : t > 0.0 ? A + log1p(exp(-t)) : B + log1p(exp(t));
    g[v] = t > 0.0 ? exp(B - out) : 1.0 / (1.0 + exp(t));
    return out;
}

// grid n_trees, kThreads threads.  work: [n_nodes] L of the sweep, then ln|Lambda_h0| (lr_prior_kernel).  A thread folds one
// node with the matrix and two vectors in private arrays of the largest degree (1.1 KiB, in scratch memory), which holds
// the kernel to a few waves per SIMD.  That is fine here: the pass is one launch of depth + 1 short steps over at most
// MTREE_MAX_NODES nodes per workgroup, its work is O(nodes D^3) against the O(rows D^2) of the Gram pass before it, and a
// step waits on its barrier, not on memory that more waves could hide.
__global__ __launch_bounds__(kThreads) void lr_sweep_kernel(Forest f, int D, int ni, int nr, int np,
                                                            int64_t* __restrict__ si, double* __restrict__ sr,
                                                            const double* __restrict__ h0, double* __restrict__ post,
                                                            double* __restrict__ g, double* __restrict__ lml,
                                                            double* __restrict__ lcm, double* __restrict__ lnp,
                                                            double* __restrict__ work) {
    const int b = blockIdx.x;
    const int lo = f.tree_off[b], hi = f.tree_off[b + 1];
    if (lo < 0 || hi > f.n_nodes || lo >= hi || D < 1 || D > kLrD) return;       // (uniform over the workgroup)
    double* L = work;
    const double lndet0 = work[f.n_nodes];
    for (int d = f.max_depth; d >= 0; --d) {
        for (int v = lo + threadIdx.x; v < hi; v += kThreads) {
            if (f.depth[v] != d) continue;
            double own = 0.0;
            if (!lr_fold_node(f, D, ni, nr, np, v, lo, hi, si, sr, h0, lndet0, post, &own)) {
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
                out = lr_mix(g, v, own, S);
            }
            L[v] = out;
            if (v == lo) lnp[b] += out;
        }
        __syncthreads();
    }
}

// ---- (h) ------------------------------------------------------------------------------------------------------------------
// V[node] = [mu (D) | W = L^-1, packed lower triangle (D (D + 1) / 2) | alpha / beta | 2 alpha], so that
// x'Lambda^-1 x = |W x|^2.
__global__ __launch_bounds__(kThreads) void lr_values_kernel(int n_nodes, int D, int np, const double* __restrict__ post,
                                                             double* __restrict__ V) {
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n_nodes || D < 1 || D > kLrD) return;
    const int T = lr_tri(D);
    const double* p = post + (int64_t)v * np;
    double* o = V + (int64_t)v * (D + T + 2);
    double A[kLrTri];
    for (int k = 0; k < T; ++k) A[k] = p[D + k];
    lr_cholesky(A, D);                         // L[i][k] = U[k][i]
    for (int i = 0; i < D; ++i) o[i] = p[i];
    double* W = o + D;
    for (int j = 0; j < D; ++j)                // column j of L^-1: L W = I by forward substitution
        for (int i = j; i < D; ++i) {
            double t = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) t -= A[lr_ut(D, k, i)] * W[lr_lt(k, j)];
            W[lr_lt(i, j)] = t / A[lr_ut(D, i, i)];
        }
    o[D + T] = p[D + T] / p[D + T + 1];
    o[D + T + 1] = 2.0 * p[D + T];
}

// One thread per row, predict_kernel's walk and folds with node values that depend on the row: p_v(x) = x . mu_v and (VAR)
// nu / lambda / (nu - 2), lambda = (alpha / beta) / (1 + |W x|^2), NaN when nu <= 2.  x is the row's dim_cont = D features.
template <typename TC, typename TK>
__global__ __launch_bounds__(kThreads) void lr_predict_kernel(Forest f, int mode, int D, const TC* __restrict__ xc,
                                                              const TK* __restrict__ xk, int64_t n,
                                                              const double* __restrict__ g, const double* __restrict__ prob,
                                                              const double* __restrict__ V, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || D < 1 || D > kLrD) return;
    const int T = lr_tri(D), VL = D + T + 2;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool want_var = mode == MTREE_PRED_VAR;
    double xr[kLrD];
    for (int j = 0; j < D; ++j) xr[j] = (double)xc[i * f.dim_cont + j];
    int nodes[MTREE_MAX_DEPTH + 1];
    double mix_mean = 0.0, acc = 0.0;
    auto value = [&](int v, bool var, double* s2) {
        const double* o = V + (int64_t)v * VL;
        double m = 0.0;
        for (int j = 0; j < D; ++j) m += xr[j] * o[j];
        if (var) {
            double q = 0.0;
            for (int a = 0; a < D; ++a) {
                double u = 0.0;
                for (int c = 0; c <= a; ++c) u += o[D + lr_lt(a, c)] * xr[c];
                q += u * u;
            }
            const double lam = o[D + T] / (1.0 + q), nu = o[D + T + 1];
            *s2 = nu > 2.0 ? nu / lam / (nu - 2.0) : nan;
        }
        return m;
    };
    const int passes = want_var ? 2 : 1;
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
            double s2 = 0.0;
            const bool var = want_var && pass == 1;
            double m = value(nodes[d], var, &s2);
            for (int j = d - 1; j >= 0; --j) {
                const int v = nodes[j];
                double vv = 0.0;
                const double gv = g[v], mv = value(v, var, &vv);
                const double mm = (1.0 - gv) * mv + gv * m;
                if (var) s2 = (1.0 - gv) * ((mm - mv) * (mm - mv) + vv) + gv * ((mm - m) * (mm - m) + s2);
                m = mm;
            }
            const double pb = prob[b];
            if (!want_var) acc += pb * m;
            else if (pass == 0) mix_mean += pb * m;
            else acc += pb * ((m - mix_mean) * (m - mix_mean) + s2);
        }
    }
    out[i] = acc;
}

}  // namespace mtree
