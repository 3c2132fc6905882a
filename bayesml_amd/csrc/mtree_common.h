// What the kernels of include/mtree.h (mtree_kernels.h, mtree_lr_kernels.h) and of include/mtpred.h (mtpred_kernels.h) share:
// the forest by value, the out-of-line lgamma, and the packed-triangle index arithmetic and Cholesky factorisation of the
// linear-regression sub-model.  No kernels here, so more than one translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtree.h"

namespace mtree {

constexpr int kWave = 64;
constexpr int kLrD = MTREE_LR_MAX_DEGREE;
constexpr int kLrTri = kLrD * (kLrD + 1) / 2;

struct Forest {        // mtree_forest by value
    int n_trees, n_nodes, n_thr, max_depth, dim_cont, dim_cat;
    const int32_t *tree_off, *feat, *child0, *nchild, *thr_off, *depth;
    const double* thr;
};

__device__ __attribute__((noinline)) inline double lgamma_call(double x) { return lgamma(x); }

__host__ __device__ inline int lr_tri(int D) { return D * (D + 1) / 2; }
// index of (i, j), i <= j, in the row-major upper triangle of a D x D matrix
__device__ inline int lr_ut(int D, int i, int j) { return i * D - i * (i - 1) / 2 + (j - i); }

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

}  // namespace mtree
