// Kernels of include/mtpred.h: the predictive log-density of labelled rows under a fixed meta-tree forest.
//
// (a) consts_kernel: one thread per node, once per call: what a visit needs of the node's posterior and y does not change.
// (b) pass_kernel<FAMILY, STAGED>: a workgroup of kWaves waves owns a tile of kTile rows.  A lane is a row; wave w takes
//     trees w, w + kWaves, ...  STAGED: all threads copy the tile's features into LDS once, feature-major ([feature][row]),
//     so the lanes of a wave that stand at one node read one feature from consecutive words and the B operand of the matrix
//     path is a plain strided read; otherwise (the tile is larger than kLdsBytes) the rows are read where they lie.  The
//     walk and the fold run over a uniform level counter, so the path is a private array under a uniform index.
//     Linear regression: lr_level() evaluates (mu . x, |W x|^2) of every active lane's node at one level - the nodes that
//     `share` lanes or more have in common on v_mfma_f64_16x16x4_f64, all other lanes in the triangular form.
// (c) total_kernel: one workgroup adds the tiles' sums, a thread over a strided slice in slice order, then a fixed LDS tree.
#pragma once
#include "common.h"
#include "mtree_common.h"

#include "../../include/mtpred.h"

namespace mtpred {
using gmmvb::d4;
using gmmvb::mfma_f64;
using mtree::Forest;
using mtree::lgamma_call;

constexpr int kTile = MTPRED_TILE;
constexpr int kWaves = MTPRED_WAVES;
constexpr int kThreads = kTile * kWaves;
constexpr int kLdsBytes = MTPRED_LDS_BYTES;
constexpr int kImg = 16;                       // the operand image of a linear-regression node is kImg x kImg
constexpr int kLrConsts = MTPRED_LR_CONSTS;
constexpr double kLnPi = 1.1447298858494002;
static_assert(kTile == mtree::kWave, "a lane is a row");
static_assert(MTREE_LR_MAX_DEGREE < kImg, "row 15 of the image holds mu");

__device__ inline double neg_inf() { return __longlong_as_double(0xfff0000000000000ll); }

// ---- (a) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void consts_kernel(int n_nodes, int family, int D, int np, int CL,
                                                     const double* __restrict__ post, double* __restrict__ consts) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_nodes) return;
    const double* p = post + (int64_t)v * np;
    double* o = consts + (int64_t)v * CL;
    if (family == MTREE_BERNOULLI) {
        const double s = p[0] + p[1];
        o[0] = log(p[0] / s);
        o[1] = log(p[1] / s);
    } else if (family == MTREE_CATEGORICAL) {
        double s = 0.0;
        for (int a = 0; a < D; ++a) s += p[a];
        for (int a = 0; a < D; ++a) o[a] = log(p[a] / s);
    } else if (family == MTREE_POISSON) {
        o[0] = lgamma_call(p[0]);
        o[1] = p[0] * log(p[1] / (1.0 + p[1]));
        o[2] = log1p(p[1]);
    } else if (family == MTREE_EXPONENTIAL) {
        o[0] = log(p[0]) + p[0] * log(p[1]);
        o[1] = p[0] + 1.0;
        o[2] = p[1];
    } else if (family == MTREE_NORMAL) {
        const double nu = 2.0 * p[2], lam = p[1] / (p[1] + 1.0) * p[2] / p[3], h = 0.5 * (nu + 1.0);
        o[0] = p[0];
        o[1] = lam / nu;
        o[2] = h;
        o[3] = lgamma_call(h) - lgamma_call(0.5 * nu) + 0.5 * (log(lam / nu) - kLnPi);
    } else {
        if (D < 1 || D > mtree::kLrD) return;
        const int T = mtree::lr_tri(D);
        double A[mtree::kLrTri];
        for (int k = 0; k < T; ++k) A[k] = p[D + k];
        mtree::lr_cholesky(A, D);               // Lambda = U'U, L = U'
        for (int k = 0; k < kImg * kImg; ++k) o[k] = 0.0;
        for (int j = 0; j < D; ++j)             // column j of W = L^-1 by forward substitution, as lr_values_kernel does
            for (int i = j; i < D; ++i) {
                double t = i == j ? 1.0 : 0.0;
                for (int k = j; k < i; ++k) t -= A[mtree::lr_ut(D, k, i)] * o[k * kImg + j];
                o[i * kImg + j] = t / A[mtree::lr_ut(D, i, i)];
            }
        for (int j = 0; j < D; ++j) o[(kImg - 1) * kImg + j] = p[j];
        const double ab = p[D + T] / p[D + T + 1], nu = 2.0 * p[D + T], h = 0.5 * (nu + 1.0);
        double* s = o + kImg * kImg;
        s[0] = ab / nu;
        s[1] = h;
        s[2] = lgamma_call(h) - lgamma_call(0.5 * nu) + 0.5 * (log(ab / nu) - kLnPi);
        s[3] = nu;
    }
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------
__device__ inline double load_cont(const void* p, int dt, int64_t k) {
    return dt == MTREE_F32 ? (double)((const float*)p)[k] : ((const double*)p)[k];
}
// a categorical value as a child index, -1 where it can be no child of any node
__device__ inline int load_cat(const void* p, int dt, int64_t k) {
    const int64_t a = dt == MTREE_U8 ? (int64_t)((const uint8_t*)p)[k]
                      : dt == MTREE_I32 ? (int64_t)((const int32_t*)p)[k] : ((const int64_t*)p)[k];
    return (uint64_t)a < (uint64_t)MTREE_MAX_CHILDREN ? (int)a : -1;
}

// The features of one tile: row r of the tile is row row0 + r of the call.
template <bool STAGED>
struct Rows {
    const double* sc;      // LDS [dim_cont][kTile]
    const int32_t* sk;     // LDS [dim_cat][kTile]
    const void *xc, *xk;
    int xc_dtype, xk_dtype, dim_cont, dim_cat;
    int64_t row0, n;
    __device__ double cont(int r, int j) const {
        if (STAGED) return sc[j * kTile + r];
        return row0 + r < n ? load_cont(xc, xc_dtype, (row0 + r) * dim_cont + j) : 0.0;
    }
    __device__ int cat(int r, int j) const {
        if (STAGED) return sk[j * kTile + r];
        return row0 + r < n ? load_cat(xk, xk_dtype, (row0 + r) * dim_cat + j) : -1;
    }
};

// mtree::next_node on a tile: the child of node v that tile row r goes to, or -1 where the walk stops.
template <bool STAGED>
__device__ inline int next_node(const Forest& f, int v, int lo, int hi, const Rows<STAGED>& rows, int r) {
    const int ft = f.feat[v], nc = f.nchild[v];
    if (ft < 0 || nc < 1 || nc > MTREE_MAX_CHILDREN || ft >= f.dim_cont + f.dim_cat) return -1;
    int child = -1;
    if (ft < f.dim_cont) {
        const int to = f.thr_off[v];
        if (to < 0 || to + nc - 1 >= f.n_thr || !f.thr) return -1;
        const double x = rows.cont(r, ft);
        if (x < f.thr[to + 1]) child = 0;
        else if (f.thr[to + nc - 1] <= x) child = nc - 1;
        else
            for (int j = 1; j + 1 < nc; ++j)
                if (f.thr[to + j] <= x && x < f.thr[to + j + 1]) {
                    child = j;
                    break;
                }
    } else {
        const int a = rows.cat(r, ft - f.dim_cont);
        if (a >= 0 && a < nc) child = a;
    }
    if (child < 0) return -1;
    const int nx = f.child0[v] + child;
    return (nx > v && nx >= lo && nx < hi) ? nx : -1;
}

// What of a row's label no node changes.
struct Label {
    double y;          // the label as binary64 (a count, a class or a real)
    int64_t k;         // the label of a discrete family
    double lg1;        // poisson: lgamma(y + 1)
    bool ok;           // inside the family's support
};

template <int FAMILY>
__device__ inline Label label_of(const long long raw, int degree) {
    Label l;
    l.k = 0;
    l.lg1 = 0.0;
    if (FAMILY <= MTREE_POISSON) {
        l.k = raw;
        l.y = (double)raw;
        l.ok = FAMILY == MTREE_BERNOULLI ? (raw == 0 || raw == 1)
               : FAMILY == MTREE_CATEGORICAL ? (uint64_t)raw < (uint64_t)degree : raw >= 0;
        if (FAMILY == MTREE_POISSON && l.ok) l.lg1 = lgamma_call(l.y + 1.0);
    } else {
        l.y = __longlong_as_double(raw);
        l.ok = FAMILY == MTREE_EXPONENTIAL ? !(l.y < 0.0) : true;
    }
    return l;
}

// ln p_v(y) of a scalar family from the node's constants c (and alpha = post[0] for poisson).
template <int FAMILY>
__device__ inline double node_logp(const double* __restrict__ c, const double* __restrict__ post_v, const Label& l) {
    if (!l.ok) return neg_inf();
    if (FAMILY == MTREE_BERNOULLI) return c[l.k == 1 ? 0 : 1];
    if (FAMILY == MTREE_CATEGORICAL) return c[l.k];
    if (FAMILY == MTREE_POISSON) return ((lgamma_call(l.y + post_v[0]) - l.lg1) - c[0]) + (c[1] - l.y * c[2]);
    if (FAMILY == MTREE_EXPONENTIAL) return c[0] - c[1] * log(c[2] + l.y);
    const double r = l.y - c[0];
    return c[3] - c[2] * log1p(c[1] * (r * r));
}

// ln p_v(y | x) of linear regression from (mean, q) = (mu . x, |W x|^2) and the node's four scalars s.
__device__ inline double lr_logp(const double* __restrict__ s, double mean, double q, double y) {
    const double r = y - mean;
    return (s[2] - 0.5 * log1p(q)) - s[1] * log1p(s[0] / (1.0 + q) * (r * r));
}

// The two-way mixture of an inner node in the log domain; g <= 0 and g >= 1 are fixed points.
__device__ inline double mix(double g, double own, double child) {
    if (!(g > 0.0)) return own;
    if (!(g < 1.0)) return child;
    const double a = log1p(-g) + own, c = log(g) + child;
    const double m = fmax(a, c);
    if (m == neg_inf()) return m;
    return m + log1p(exp(-fabs(a - c)));
}

// (mean, q) of node v for every lane with `active`, one level of one tree.  All 64 lanes of the wave call it together.
template <bool STAGED>
__device__ inline void lr_level(const Rows<STAGED>& rows, int D, const double* __restrict__ consts, int n_nodes, int v,
                                bool active, int share, double* mean_out, double* q_out) {
    const int lane = threadIdx.x & 63, col = lane & 15, grp = lane >> 4;
    active = active && v >= 0 && v < n_nodes;
    double mean = 0.0, q = 0.0;
    bool pending = active;
    unsigned long long rest = __ballot(active);
    while (rest) {
        const int lead = __ffsll((long long)rest) - 1;
        const int v0 = __shfl(v, lead);
        const bool in = active && v == v0;
        const unsigned long long same = __ballot(in);
        rest &= ~same;
        if (__popcll(same) < share) continue;
        // image (16 x 16) times X' (16 x 64): lane l supplies A[l & 15][4 kk + (l >> 4)] and B[4 kk + (l >> 4)][l & 15]
        const double* img = consts + (int64_t)v0 * kLrConsts;
        double a[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) a[kk] = img[col * kImg + 4 * kk + grp];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = 4 * kk + grp;
                acc = mfma_f64(a[kk], k < D ? rows.cont(cb * 16 + col, k) : 0.0, acc);
            }
            // acc[r] = (image x)[grp + 4 r] of tile row cb * 16 + col: the squares of rows < D, then the groups 0+1, 2+3
            double qq = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) qq += grp + 4 * r < D ? acc[r] * acc[r] : 0.0;
            qq += __shfl_xor(qq, 16);
            qq += __shfl_xor(qq, 32);
            const double mm = __shfl(acc[3], 48 + col);
            if (in && grp == cb) {
                q = qq;
                mean = mm;
            }
        }
        pending = pending && !in;
    }
    if (pending) {      // lr_predict_kernel's arithmetic on the image
        const double* img = consts + (int64_t)v * kLrConsts;
        for (int j = 0; j < D; ++j) mean += rows.cont(lane, j) * img[(kImg - 1) * kImg + j];
        for (int a = 0; a < D; ++a) {
            double u = 0.0;
            for (int c = 0; c <= a; ++c) u += img[a * kImg + c] * rows.cont(lane, c);
            q += u * u;
        }
    }
    *mean_out = mean;
    *q_out = q;
}

// grid: tiles, kThreads threads; dynamic LDS: kTile * (8 dim_cont + 4 dim_cat) bytes when STAGED.
template <int FAMILY, bool STAGED>
__global__ __launch_bounds__(kThreads) void pass_kernel(Forest f, int degree, int np, int CL, int xc_dtype,
                                                        const void* __restrict__ xc, int xk_dtype,
                                                        const void* __restrict__ xk, const long long* __restrict__ y,
                                                        int64_t n, const double* __restrict__ post,
                                                        const double* __restrict__ g, const double* __restrict__ prob,
                                                        const double* __restrict__ consts, int share,
                                                        double* __restrict__ lnp, double* __restrict__ tile_sum) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ long long sy[kTile];
    __shared__ double part_m[kWaves][kTile], part_s[kWaves][kTile];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    const int rows_here = (int)(n - row0 < kTile ? n - row0 : kTile);
    double* sc = (double*)lds;
    int32_t* sk = (int32_t*)(lds + sizeof(double) * (size_t)kTile * f.dim_cont);
    if (STAGED) {
        // the tile's rows are one contiguous block of either matrix; rows past n are zeros (no child, 0.0)
        for (int e = tid; e < kTile * f.dim_cont; e += kThreads) {
            const int r = e / f.dim_cont, j = e - r * f.dim_cont;
            sc[j * kTile + r] = r < rows_here ? load_cont(xc, xc_dtype, row0 * f.dim_cont + e) : 0.0;
        }
        for (int e = tid; e < kTile * f.dim_cat; e += kThreads) {
            const int r = e / f.dim_cat, j = e - r * f.dim_cat;
            sk[j * kTile + r] = r < rows_here ? load_cat(xk, xk_dtype, row0 * f.dim_cat + e) : -1;
        }
    }
    if (tid < kTile) sy[tid] = tid < rows_here ? y[row0 + tid] : 0ll;
    __syncthreads();
    const Rows<STAGED> rows = {sc, sk, xc, xk, xc_dtype, xk_dtype, f.dim_cont, f.dim_cat, row0, n};
    const bool valid = lane < rows_here;
    const Label lab = label_of<FAMILY>(sy[lane], degree);
    const int maxd = f.max_depth < MTREE_MAX_DEPTH ? f.max_depth : MTREE_MAX_DEPTH;

    int nodes[MTREE_MAX_DEPTH + 1];
    double mx = neg_inf(), sum = 0.0;          // the wave's trees so far: sum of exp(ln prob_b + value_b - mx)
    bool nan_seen = false;
    for (int b = w; b < f.n_trees; b += kWaves) {
        const double pb = prob[b];
        const int lo = f.tree_off[b], hi = f.tree_off[b + 1];
        if (!(pb > 0.0) || lo < 0 || hi > f.n_nodes || lo >= hi) continue;      // (uniform over the wave)
        // the walk: nodes[0..d], level by level
        int d = 0, cur = lo;
        bool alive = valid;
        nodes[0] = lo;
        for (int lv = 0; lv < maxd; ++lv) {
            if (alive) {
                const int nx = next_node<STAGED>(f, cur, lo, hi, rows, lane);
                if (nx < 0) alive = false;
                else {
                    cur = nx;
                    d = lv + 1;
                }
            }
            nodes[lv + 1] = cur;
            if (!__any(alive)) break;
        }
        // the fold, from the deepest level up; a lane joins at its stop node
        double val = 0.0;
        for (int j = maxd; j >= 0; --j) {
            const bool at = valid && j <= d;
            if (!__any(at)) continue;
            const int v = at ? nodes[j] : -1;
            double own;
            if (FAMILY == MTREE_LINREG) {
                double mean, q;
                lr_level<STAGED>(rows, degree, consts, f.n_nodes, v, at, share, &mean, &q);
                own = at ? lr_logp(consts + (int64_t)v * kLrConsts + kImg * kImg, mean, q, lab.y) : 0.0;
            } else {
                own = at ? node_logp<FAMILY>(consts + (int64_t)v * CL, post + (int64_t)v * np, lab) : 0.0;
            }
            if (at) val = j == d ? own : mix(g[v], own, val);
        }
        const double lt = log(pb) + val;
        if (lt > mx) {
            sum = sum * exp(mx - lt) + 1.0;
            mx = lt;
        } else if (lt != neg_inf()) {
            sum += exp(lt - mx);
        }
        nan_seen = nan_seen || lt != lt;
    }
    // (a NaN value, from a NaN label or feature, stays a NaN through the maxima below)
    part_m[w][lane] = nan_seen ? __longlong_as_double(0x7ff8000000000000ll) : mx;
    part_s[w][lane] = sum;
    __syncthreads();
    if (w != 0) return;
    double top = part_m[0][lane];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
        const double m = part_m[k][lane];
        top = (m > top || m != m) ? m : top;
    }
    double out = top;
    if (top != neg_inf()) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k)
            if (part_m[k][lane] != neg_inf()) s += part_s[k][lane] * exp(part_m[k][lane] - top);
        out = top + log(s);
    }
    if (valid) lnp[row0 + lane] = out;
    if (tile_sum) {
        double t = valid ? out : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0) tile_sum[blockIdx.x] = t;
    }
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void total_kernel(const double* __restrict__ tile_sum, int64_t tiles,
                                                    double* __restrict__ total) {
    __shared__ double part[256];
    double acc = 0.0;
    for (int64_t k = threadIdx.x; k < tiles; k += 256) acc += tile_sum[k];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = part[0];
}

}  // namespace mtpred
