/*
 * regpred.h — C ABI of the held-out scoring and many-series passes of the Normal-Gamma regression family on the MI355X
 * (gfx950), in libgmmvb.so beside regvb.h.
 *
 * Under a fixed posterior (mu, Lambda = L L^T, alpha, beta) the predictive density of a target y with regressors w is the
 * Student-t of bayesml/linearregression/_linearregression.py:716-720,
 *
 *     m = w . mu,   lambda = scale / (1 + |L^-1 w|^2),   scale = alpha / beta,   nu = 2 alpha,
 *     ln p = c0 + ln(lambda) / 2 - (nu + 1) / 2 * log1p(lambda (y - m)^2 / nu),
 *     c0 = lnGamma((nu + 1) / 2) - lnGamma(nu / 2) - ln(pi nu) / 2     (the caller's, in binary64).
 *
 * regpred_logpdf writes ln p of every row in one fused pass (no p_ms / p_lambdas arrays exist); regpred_logpdf_window does
 * the same for the lag windows of n_seq independent series laid end to end, and regpred_stats_window accumulates the
 * statistics block of regvb.h over those windows.  No window reaches before the start of its own series.
 *
 * The rows of the series.  Series s holds the values off[s] .. off[s + 1] - 1 of the array.  With REGVB_PAD_ZEROS every
 * value is a row (values before the series' own start read as zero); with REGVB_PAD_NONE the first p values of a series
 * are initial values only and a series of at most p values has no row.  Rows are numbered series after series:
 * roff[s] is the number of rows of the series before s, roff[n_seq] = n_rows.  Both tables are the caller's, [n_seq + 1]
 * int64 in device memory; that they ascend and agree with each other, with `length` and with n_rows is the caller's
 * contract (it cannot be checked without reading device memory).  No n_rows-sized index array is built or read: a
 * workgroup finds the series of its rows by bisection of roff.
 *
 * Conventions are regvb.h's: *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = the null stream); calls only enqueue, never allocate, never synchronise; the return value is a status code and
 * regpred_last_error() gives a thread-local message.  Arguments are validated before anything touches the device.  Rows
 * stay in their storage dtype and are widened on load; every sum and output is IEEE binary64.  No atomics: two calls on
 * the same input give the same bits.  D <= REGPRED_MAX_DEGREE features; beyond that REGPRED_EUNSUPPORTED.
 */
#ifndef REGPRED_H
#define REGPRED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REGPRED_ABI_VERSION 1
#define REGPRED_MAX_DEGREE 256
#define REGPRED_TOTAL_CHUNK 4096 /* rows per first-level partial sum of the grand total */

enum regpred_status { REGPRED_OK = 0, REGPRED_EINVAL = 1, REGPRED_EUNSUPPORTED = 2, REGPRED_EHIP = 3 };
enum regpred_dtype { REGPRED_F32 = 0, REGPRED_F64 = 1 };
enum regpred_padding { REGPRED_PAD_NONE = 0, REGPRED_PAD_ZEROS = 1 };

int regpred_abi_version(void);
const char* regpred_last_error(void);

/* Doubles of scratch of regpred_logpdf / regpred_logpdf_window for D features: the inverse factor packed in operand
 * order (-1 for D outside 1..256). */
int64_t regpred_work_len(int D);

/* lnp[n] = ln p(y_n | x_n) for the rows x[n_rows][D] (x_dtype, row stride ldx >= D elements) and targets y[n_rows]
 * (y_dtype); the two dtypes are independent.  mu_dev [D]; linv_dev [D][D] row-major lower triangular, the inverse Cholesky
 * factor of Lambda (the strict upper triangle is not read); scale, nu > 0. */
int regpred_logpdf(int D, int x_dtype, const void* x_dev, int64_t ldx, int y_dtype, const void* y_dev, int64_t n_rows,
                   const double* mu_dev, const double* linv_dev, double scale, double nu, double c0, double* lnp_dev,
                   double* work_dev, void* stream);

/* The same for the n_rows lag windows [1, x[t-p], ..., x[t-1]] -> x[t] of the n_seq series in series[length] (D = p + 1;
 * see "The rows of the series" above). */
int regpred_logpdf_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding, int64_t n_seq,
                          const int64_t* off_dev, const int64_t* roff_dev, int64_t n_rows, const double* mu_dev,
                          const double* linv_dev, double scale, double nu, double c0, double* lnp_dev, double* work_dev,
                          void* stream);

/* Doubles of scratch of regpred_stats_window for D features (regvb_stats_work_len's: one slab per workgroup). */
int64_t regpred_stats_work_len(int D);

/* The statistics block [ G | c | s | n ] of regvb.h (regvb_stats_len(p + 1) doubles) over the same n_rows windows: what
 * the sum of regvb_stats_window over the series gives, to rounding, in one pass.  Slabs are added in split order. */
int regpred_stats_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding, int64_t n_seq,
                         const int64_t* off_dev, const int64_t* roff_dev, int64_t n_rows, double* stats_dev,
                         double* work_dev, void* stream);

/* Doubles of scratch of regpred_totals with a grand total over n_rows rows (-1 for n_rows < 0). */
int64_t regpred_totals_work_len(int64_t n_rows);

/* tot[s] = sum of lnp[roff[s] .. roff[s + 1]) (0.0 for a series without rows) and total[0] = sum of lnp[0 .. n_rows), each
 * by one fixed-shape tree: a wave per segment adds 64 strided partial sums and closes with a butterfly; the grand total
 * does so over chunks of REGPRED_TOTAL_CHUNK rows and then over the chunk sums.  tot_dev (with roff_dev, n_seq >= 1) and
 * total_dev (with work_dev) may each be NULL. */
int regpred_totals(int64_t n_seq, const int64_t* roff_dev, int64_t n_rows, const double* lnp_dev, double* tot_dev,
                   double* total_dev, double* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REGPRED_H */
