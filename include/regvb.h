/*
 * regvb.h — C ABI of the Normal-Gamma regression data passes on the MI355X (gfx950), in libgmmvb.so beside gmmvb.h.
 *
 * The reference (bayesml/BayesML v0.3.1) is pure Python; these entry points are what a binding of
 * linearregression.LearnModel and autoregressive.LearnModel calls in place of the NumPy code that touches N-sized data:
 *
 *   x.T @ x, x.T @ y, y @ y            bayesml/linearregression/_linearregression.py:544-548   (regvb_stats)
 *   x_mat loop + the same sums         bayesml/autoregressive/_autoregressive.py:481-503        (regvb_stats_window)
 *   x @ mu, x^T Lambda^-1 x per row    bayesml/linearregression/_linearregression.py:717-718   (regvb_predict)
 *
 * Conventions are gmmvb.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise;
 * the return value is a status code (same values as enum gmmvb_status) and regvb_last_error() gives a thread-local
 * message.  Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 * Rows stay in their storage dtype (f32 or f64) and are widened on load; every sum and every output is IEEE binary64.
 * All kernels are f64 MFMA kernels for D <= REGVB_MAX_DEGREE features; a larger D returns REGVB_EUNSUPPORTED.
 * No sum uses atomics: two calls on the same input give the same bits.
 */
#ifndef REGVB_H
#define REGVB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REGVB_ABI_VERSION 1
#define REGVB_MAX_DEGREE 256

enum regvb_status { REGVB_OK = 0, REGVB_EINVAL = 1, REGVB_EUNSUPPORTED = 2, REGVB_EHIP = 3 };
enum regvb_dtype { REGVB_F32 = 0, REGVB_F64 = 1 };
enum regvb_padding { REGVB_PAD_NONE = 0, REGVB_PAD_ZEROS = 1 };

int regvb_abi_version(void);
const char* regvb_last_error(void);

/* Doubles in a statistics block of D features:  [ G[D][D] | c[D] | s | n ]  (D*D + D + 2; -1 for D outside 1..256)
 *   G = sum_n w_n w_n^T (full, exactly symmetric), c = sum_n w_n y_n, s = sum_n y_n^2, n = number of rows.
 * The block is linear in the rows: the blocks of two row ranges add to the block of their union. */
int64_t regvb_stats_len(int D);
/* Doubles of scratch regvb_stats / regvb_stats_window need for D features: one slab of partial sums per workgroup, as many
 * slabs as the GPU holds workgroups.  Independent of n_rows but not small: about 10 MB up to D = 32, 32 MB to 64, 45 MB
 * to 96, 57 MB to 128, then 29, 41, 55 and 71 MB for D up to 160, 192, 224 and 256. */
int64_t regvb_stats_work_len(int D);

/* Statistics of the rows x[n_rows][D] of dtype x_dtype (row stride ldx >= D elements) with targets y[n_rows] of dtype
 * y_dtype.  The two dtypes are independent: each value is widened to binary64 on load, none is narrowed. */
int regvb_stats(int D, int x_dtype, const void* x_dev, int64_t ldx, int y_dtype, const void* y_dev, int64_t n_rows,
                double* stats_dev, double* work_dev, void* stream);

/* The same for the lag windows of a series x[length] of degree p (D = p + 1): row t is [1, x[t-p], ..., x[t-1]], target
 * x[t]; t = p .. length-1 (REGVB_PAD_NONE) or t = 0 .. length-1 with zeros at negative times (REGVB_PAD_ZEROS).
 * length > p.  The [length, p+1] matrix is never materialised. */
int regvb_stats_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding,
                       double* stats_dev, double* work_dev, void* stream);

/* Doubles of scratch regvb_predict needs for D features (the factor packed in operand order). */
int64_t regvb_predict_work_len(int D);

/* Per row of x[n_rows][D]:  p_ms[n] = x_n . mu,  p_lambdas[n] = scale / (1 + |Linv x_n|^2), where Linv [D][D] (row-major,
 * lower triangular; the strict upper triangle is not read) is the inverse Cholesky factor of Lambda = L L^T and
 * scale = alpha / beta. */
int regvb_predict(int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* mu_dev,
                  const double* linv_dev, double scale, double* p_ms_dev, double* p_lambdas_dev, double* work_dev,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REGVB_H */
