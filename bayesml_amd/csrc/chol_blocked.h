// Factor and invert in blocks of 16 on v_mfma_f64_16x16x4_f64: what the K-side kernels (kside.hip, D > 32) and the block
// kernels of sequential regression (regseq_kernels.h) share.  Device only.
#pragma once
#include "common.h"

namespace gmmvb {

// ---- factor and invert in blocks of 16 on v_mfma_f64_16x16x4_f64 (D > 32) ----------------------------------------------
// The matrix lives in LDS as [PD][PD + 1] doubles, PD = D rounded up to 16, lower triangle filled, the rest zero, with an
// identity corner in the padding (rows and columns >= D): no lane ever takes the square root or the reciprocal of a
// padding zero, and the padding never mixes with the D x D part.  dinv [PD / 16][16][17] receives the inverses of the
// factor's diagonal blocks.  NW waves (64 NW threads) call these together; tiles are dealt out per wave.
// MFMA lane map (lane l: li = l & 15, lg = l >> 4): a = X[li][p + lg], b = Y[p + lg][li], result register r is row
// lg + 4 r, column li of the tile.
constexpr int kDinvLd = 17, kDinvSize = 16 * kDinvLd;

__device__ __forceinline__ double lane_bcast(double v, int src) {          // src: a constant after unrolling
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// One wave: Cholesky of the 16 x 16 diagonal block at (j0, j0) in registers - lane i (and its three copies i + 16 g, which
// compute the same and store nothing) holds row i; the column steps are those of the unblocked loop, with lane
// broadcasts instead of barriers - then the block's inverse, lane j holding column j.  A non-positive pivot leaves NaN
// in its column and in everything right of and below it, as the unblocked loop does.
__device__ __forceinline__ void diag_block_factor(double* mat, int ld, int j0, double* dinv) {
    const int lane = threadIdx.x & 63, i = lane & 15;
    double x[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = c <= i ? mat[(j0 + i) * ld + j0 + c] : 0.0;
    double inv_own = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double d = sqrt(lane_bcast(x[j], j));
        const double inv = 1.0 / d;
        x[j] = i == j ? d : (i > j ? x[j] * inv : 0.0);
        inv_own = i == j ? inv : inv_own;
#pragma unroll
        for (int c = j + 1; c < 16; ++c) x[c] = fma(-x[j], lane_bcast(x[j], c), x[c]);      // (used for i >= c only)
    }
    if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 16; ++c) mat[(j0 + i) * ld + j0 + c] = x[c];
    }
    // inverse by forward substitution, column i of it in lane i: z[r] = -(sum_{p < r} L[r][p] z[p]) / L[r][r], with L[r][p]
    // read back from LDS (one address for the whole wave), so that x[] need not stay in registers beside z[]
    double z[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const double inv_r = lane_bcast(inv_own, r);
        double s = 0.0;
#pragma unroll
        for (int p = 0; p < r; ++p) s = fma(mat[(j0 + r) * ld + j0 + p], z[p], s);
        z[r] = i < r ? -s * inv_r : (i == r ? inv_r : 0.0);
    }
    if (lane < 16) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dinv[r * kDinvLd + i] = z[r];
    }
}

// Right-looking Cholesky, NB = 16: the diagonal block in one wave's registers, the panel below it as A21 L11^-T and the
// trailing update C -= L21 L21^T over the lower tiles on the matrix pipe (the tile is the MFMA's C operand and -L21 its A
// operand, so every element is still fma(-l_ij, l_cj, a_ic) column by column).  Wave 0 takes the next diagonal tile of
// the trailing update and factorises it at once, beside the other waves' tiles: two barriers per block.
// SUBST: the panel by forward substitution on L11, a thread per row, instead of the product with L11^-1.  The product's
// backward error grows with cond(L11); the substitution's does not (regseq_kernels.h factorises Lambda_0 + G under a
// diffuse prior, where the leading blocks are nearly singular until D rows have been seen).
template <int NW, bool SUBST = false>
__device__ __forceinline__ void blocked_cholesky(double* mat, int ld, int ntl, double* dinv) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    auto syrk_tile = [&](int rt, int ct, int j0) {
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mat[(16 * rt + lg + 4 * r) * ld + 16 * ct + li];
#pragma unroll
        for (int p = 0; p < 16; p += 4)
            acc = mfma_f64(-mat[(16 * rt + li) * ld + j0 + p + lg], mat[(16 * ct + li) * ld + j0 + p + lg], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) mat[(16 * rt + lg + 4 * r) * ld + 16 * ct + li] = acc[r];
    };
    for (int kb = 0; kb < ntl; ++kb) {
        if (wv == 0) {
            if (kb > 0) syrk_tile(kb, kb, 16 * (kb - 1));
            diag_block_factor(mat, ld, 16 * kb, dinv + kb * kDinvSize);
        } else if (kb > 0) {
            int t = 0;
            for (int rt = kb + 1; rt < ntl; ++rt)
                for (int ct = kb; ct <= rt; ++ct, ++t)
                    if (t % (NW - 1) == wv - 1) syrk_tile(rt, ct, 16 * (kb - 1));
        }
        __syncthreads();
        const int j0 = 16 * kb;
        if constexpr (SUBST) {
            for (int row = 16 * (kb + 1) + (int)threadIdx.x; row < 16 * ntl; row += 64 * NW) {      // x L11^T = a
                double x[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    double s = mat[row * ld + j0 + c];
#pragma unroll
                    for (int p = 0; p < c; ++p) s = fma(-x[p], mat[(j0 + c) * ld + j0 + p], s);
                    x[c] = s / mat[(j0 + c) * ld + j0 + c];
                }
#pragma unroll
                for (int c = 0; c < 16; ++c) mat[row * ld + j0 + c] = x[c];
            }
            __syncthreads();
            continue;
        }
        const double* di = dinv + kb * kDinvSize;
        for (int rt = kb + 1 + wv; rt < ntl; rt += NW) {          // panel: L21 = A21 L11^-T
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int p = 0; p < 16; p += 4)
                acc = mfma_f64(mat[(16 * rt + li) * ld + j0 + p + lg], di[li * kDinvLd + p + lg], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) mat[(16 * rt + lg + 4 * r) * ld + j0 + li] = acc[r];
        }
        __syncthreads();
    }
}

// In-place inverse of the blocked factor: the diagonal blocks' inverses exist (dinv); T = G21 X11 for every block column
// in one pass, then block column by block column, last first, X21 = -X22 T with X22 already inverted.  Everybody must
// have finished reading the factor before the call.
template <int NW>
__device__ __forceinline__ void blocked_tri_inverse(double* mat, int ld, int ntl, const double* dinv) {
    static_assert(NW >= 8, "one wave per tile row of a block column");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    for (int kb = wv; kb < ntl; kb += NW) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            mat[(16 * kb + lg + 4 * r) * ld + 16 * kb + li] = dinv[kb * kDinvSize + (lg + 4 * r) * kDinvLd + li];
    }
    {
        int t = 0;
        for (int kb = 0; kb + 1 < ntl; ++kb)
            for (int rt = kb + 1; rt < ntl; ++rt, ++t) {
                if (t % NW != wv) continue;
                const double* di = dinv + kb * kDinvSize;
                d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int p = 0; p < 16; p += 4)
                    acc = mfma_f64(mat[(16 * rt + li) * ld + 16 * kb + p + lg], di[(p + lg) * kDinvLd + li], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) mat[(16 * rt + lg + 4 * r) * ld + 16 * kb + li] = acc[r];
            }
    }
    __syncthreads();
    for (int kb = ntl - 2; kb >= 0; --kb) {
        const int rt = kb + 1 + wv;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
        if (rt < ntl) {
            for (int ct = kb + 1; ct <= rt; ++ct)
#pragma unroll
                for (int p = 0; p < 16; p += 4)
                    acc = mfma_f64(-mat[(16 * rt + li) * ld + 16 * ct + p + lg], mat[(16 * ct + p + lg) * ld + 16 * kb + li], acc);
        }
        __syncthreads();
        if (rt < ntl) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mat[(16 * rt + lg + 4 * r) * ld + 16 * kb + li] = acc[r];
        }
        __syncthreads();
    }
}

// The same inverse block row by block row, as the solution of L X = I:  L_rr X[rt][ct] = -sum_{k = ct}^{rt - 1} L[rt][k] X[k][ct],
// the sums on the matrix pipe, L_rr applied by forward substitution (all four lane groups solve column li, as in
// diag_block_factor).  |L X - I| stays of the size of eps |L| |X| however ill-conditioned the diagonal blocks are, which the
// products with their inverses above do not give.  One tile per wave and block row: ntl <= NW.
template <int NW>
__device__ __forceinline__ void blocked_tri_inverse_subst(double* mat, int ld, int ntl, const double* dinv) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    for (int rt = 1; rt < ntl; ++rt) {
        const int ct = wv;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
        if (ct < rt) {
            for (int k = ct; k < rt; ++k) {
                // (X[k][k] is still L[k][k] in memory: its inverse comes from dinv)
#pragma unroll
                for (int p = 0; p < 16; p += 4) {
                    const double b = k == ct ? dinv[k * kDinvSize + (p + lg) * kDinvLd + li] : mat[(16 * k + p + lg) * ld + 16 * ct + li];
                    acc = mfma_f64(-mat[(16 * rt + li) * ld + 16 * k + p + lg], b, acc);
                }
            }
        }
        __syncthreads();                 // everybody has read block row rt of L
        if (ct < rt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mat[(16 * rt + lg + 4 * r) * ld + 16 * ct + li] = acc[r];
            double y[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double s = mat[(16 * rt + r) * ld + 16 * ct + li];
#pragma unroll
                for (int p = 0; p < r; ++p) s = fma(-mat[(16 * rt + r) * ld + 16 * rt + p], y[p], s);
                y[r] = s / mat[(16 * rt + r) * ld + 16 * rt + r];
            }
            if (lane < 16) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mat[(16 * rt + r) * ld + 16 * ct + li] = y[r];
            }
        }
        __syncthreads();
    }
    for (int kb = wv; kb < ntl; kb += NW) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            mat[(16 * kb + lg + 4 * r) * ld + 16 * kb + li] = dinv[kb * kDinvSize + (lg + 4 * r) * kDinvLd + li];
    }
    __syncthreads();
}

}  // namespace gmmvb
