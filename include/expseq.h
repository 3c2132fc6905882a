/*
 * expseq.h — C ABI of the scalar conjugate families' prequential pass on the MI355X (gfx950), in libgmmvb.so beside
 * expfam.h.
 *
 * The reference (bayesml/BayesML v0.3.1) scores a sample prequentially one value at a time: pred_and_update(x_i) predicts
 * x_i from the posterior of x_0 .. x_{i-1} and then learns it.  For the conjugate families that posterior is the start
 * posterior plus the sufficient statistics of the earlier values, so these entry points return the predictive parameters
 * of EVERY position and the code lengths  nats[i] = -ln p(x_i | x_0 .. x_{i-1})  in one pass: an exclusive prefix scan of
 * the statistics over the sample and a closed form per position (csrc/expseq_kernels.h).
 *
 *   bernoulli    S_i = (ones, zeros)            a = alpha + ones, b = beta + zeros;  p_theta = a / (a + b)
 *                                               nats = -ln((x ? a : b) / (a + b))
 *   poisson      S_i = sum                      p_r = alpha + sum;  p_theta = 1 / (1 + (beta + i))
 *                                               nats = -[lnG(x + r) - lnG(r) - lnG(x + 1) - r log1p(1 / b) - x log1p(b)], b = beta + i
 *   exponential  S_i = sum (binary64)           p_kappa = alpha + i;  p_lambda = beta + sum
 *                                               nats = -[ln k - ln(l + x) - k log1p(x / l)]
 *   categorical  S_i = count of every category  a_k = alpha_k + count_k, s = sum(alpha) + i;  row = a / s;  nats = -ln(a_x / s)
 *   normal       S_i = (i, mean, m2) of x - x_0 (m, kappa, alpha, beta)_i = the Normal-Gamma update by S_i;
 *                                               p_mu = m_i, p_nu = 2 alpha_i, p_lambda = kappa_i / (kappa_i + 1) alpha_i / beta_i
 *                                               nats = lnG(nu / 2) - lnG((nu + 1) / 2) + ln(pi nu / l) / 2
 *                                                      + (nu + 1) / 2 log1p(l (x - mu)^2 / nu)
 *
 * Every integer statistic is exact; lnG differences are taken from the difference of the Stirling series once their
 * arguments reach 64, never from two rounded lgamma values.  The sample is read twice, every requested array is written
 * once.
 *
 * Conventions are expfam.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the
 * return value is a status code and expseq_last_error() gives a thread-local message.  Arguments are validated before
 * anything touches the device, so bad arguments are reported without a GPU.  `start` is a HOST array, read before the
 * call returns.  Every output array is optional (NULL = not computed, nothing written); the rest are binary64 [n].
 *
 * A value outside the family's domain (expfam.h) is counted in status_dev[0] (int64), adds nothing to any statistic, is
 * never used as an index and gets a NaN code length; it still occupies its position i.  The normal family has no domain
 * and always reports 0.
 *
 * No floating-point atomics and no waiting between workgroups: a workgroup owns a tile of EXPSEQ_TILE consecutive positions, one
 * workgroup of EXPSEQ_SCAN_THREADS threads scans the tiles' aggregates, and every sum is taken in one fixed tree that
 * depends on n alone.  Two calls on the same input give the same bits.
 */
#ifndef EXPSEQ_H
#define EXPSEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXPSEQ_ABI_VERSION 1
#define EXPSEQ_TILE 2048
#define EXPSEQ_SCAN_THREADS 256

enum expseq_status { EXPSEQ_OK = 0, EXPSEQ_EINVAL = 1, EXPSEQ_EUNSUPPORTED = 2, EXPSEQ_EHIP = 3 };
enum expseq_family {
    EXPSEQ_BERNOULLI = 0, EXPSEQ_POISSON = 1, EXPSEQ_EXPONENTIAL = 2, EXPSEQ_NORMAL = 3, EXPSEQ_CATEGORICAL = 4
};

int expseq_abi_version(void);
const char* expseq_last_error(void);

/* 8-byte slots of scratch for a call on m positions.  The four scalar families (degree = 0): an aggregate and a carry of 4
 * slots per tile.  EXPSEQ_CATEGORICAL (1 <= degree <= EXPFAM_MAX_DEGREE): degree + 1 slots per tile (the tile histograms
 * and the tiles' bad counts) and m row indices.  -1 for an unknown family, a degree outside the family's, or m < 1. */
int64_t expseq_work_len(int family, int degree, int64_t m);

/* `dtype` is an enum expfam_dtype: the integer families read EXPFAM_U8, EXPFAM_I32 or EXPFAM_I64, the float families
 * EXPFAM_F32 or EXPFAM_F64 (widened exactly).  x_dev must be aligned to its element size; n >= 1.  status_dev (one int64)
 * and work_dev (expseq_work_len slots) are required. */

/* start = { hn_alpha, hn_beta } */
int expseq_bernoulli(int dtype, const void* x_dev, int64_t n, const double* start, double* p_theta_dev, double* nats_dev,
                     int64_t* status_dev, void* work_dev, void* stream);
/* start = { hn_alpha, hn_beta } */
int expseq_poisson(int dtype, const void* x_dev, int64_t n, const double* start, double* p_r_dev, double* p_theta_dev,
                   double* nats_dev, int64_t* status_dev, void* work_dev, void* stream);
/* start = { hn_alpha, hn_beta } */
int expseq_exponential(int dtype, const void* x_dev, int64_t n, const double* start, double* p_kappa_dev,
                       double* p_lambda_dev, double* nats_dev, int64_t* status_dev, void* work_dev, void* stream);
/* start = { hn_m, hn_kappa, hn_alpha, hn_beta } */
int expseq_normal(int dtype, const void* x_dev, int64_t n, const double* start, double* p_mu_dev, double* p_nu_dev,
                  double* p_lambda_dev, double* nats_dev, int64_t* status_dev, void* work_dev, void* stream);

/* categorical: one CHUNK of m positions, i0 positions of the same call before it (the caller cuts a long sample so that the
 * scratch, which alone grows with both m and degree, stays bounded; the carried state is integer, so the cut changes no
 * bit).  x_dev holds indices 0 <= x < degree (onehot = 0; ld is ignored), or one-hot rows x[m][degree] with row stride
 * ld >= degree elements (onehot = 1; a row with a negative entry or a sum other than 1 is bad).
 *   alpha_dev   hn_alpha_vec [degree] of the START of the call (binary64, device; the same for every chunk)
 *   s0          its sum, taken by the caller
 *   counts_dev  int64 [degree] (device): the occurrences in the i0 positions before the chunk (zeros for the first
 *               chunk); on return those before the next chunk
 *   nats_dev    [m]          -ln(a / s),  a = alpha[x_i] + (earlier occurrences of x_i),  s = s0 + (i0 + i)
 *   rows_dev    [m][degree]  (alpha[k] + (earlier occurrences of k)) / s
 *   argmax_dev  [m] int64    the first maximum of that row (the row itself is not stored for it)
 * status_dev[0] is set by the chunk with i0 = 0 and added to by the others. */
int expseq_categorical(int dtype, const void* x_dev, int64_t m, int degree, int onehot, int64_t ld, const double* alpha_dev,
                       double s0, int64_t i0, int64_t* counts_dev, double* nats_dev, double* rows_dev, int64_t* argmax_dev,
                       int64_t* status_dev, void* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXPSEQ_H */
