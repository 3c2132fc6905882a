/*
 * hmmpred.h — C ABI of the predictive log-density of a SEQUENCE under a hidden Markov model with Student-t emissions on
 * the MI355X (gfx950), in libgmmvb.so beside stmix.h.
 *
 * K states, D dimensions; A [K][K] row-stochastic, w0 [K] the state distribution of the first row, and per state mu_k,
 * nu_k > 0 and lower triangular U_k with U_k^T U_k = Lambda_k.  For the rows x_0 .. x_{T-1}
 *
 *     ln e_tk = c_k - a_k log1p(q_tk / nu_k),   q_tk = || U_k (x_t - mu_k) ||^2,   a_k = (nu_k + D) / 2
 *     c_k     = lnGamma(a_k) - lnGamma(nu_k / 2) - (D / 2) ln(nu_k pi) + sum_j ln U_k[j][j]
 *     m_t     = max_k ln e_tk,   rho'_tk = exp(ln e_tk - m_t)
 *     w_t     = phi_{t-1} A  (t >= 1),  w_0 given
 *     s_t     = sum_k w_tk rho'_tk,   ln p_t = ln s_t + m_t,   phi_t = w_t o rho'_t / s_t
 *     z_t     = the first k that maximises phi_tk
 *
 * ln p_t = ln p(x_t | x_0 .. x_{t-1}), sum_t ln p_t is the log predictive of the sequence and phi the filtered state
 * posterior.  The emission runs on the f64 matrix pipe over stmix_pack's parameter image (D <= 128; a plain f64 kernel
 * above), the recursion chunk-parallel up to 64 states with chunk starts from short sweeps, a device-side gate and a
 * serial repair walk behind it, and as one serial walk for 65 .. 256 states ("Predictive log-density of a
 * sequence").
 *
 * Conventions are stmix.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream); calls only enqueue work, never allocate, never synchronise; the return value is a
 * status code and hmmpred_last_error() gives a thread-local message.  Arguments are validated before anything touches
 * the device, so bad arguments are reported without a GPU.
 *
 * No atomics; two calls give the same bits.  Nothing past entry T - 1 of lnp / z and entry K - 1 of end is written.
 */
#ifndef HMMPRED_H
#define HMMPRED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMMPRED_ABI_VERSION 1
#define HMMPRED_MAX_DEGREE 19200  /* stmix.h's: above 128 a plain f64 emission */
#define HMMPRED_MAX_STATES 256    /* 1 .. 64 chunk-parallel, 65 .. 256 one serial walk */
#define HMMPRED_PARALLEL_STATES 64
#define HMMPRED_MIN_CHUNK 8       /* smallest chunk_len; hmmpred_scratch_len holds boundary vectors for it */

enum hmmpred_status { HMMPRED_OK = 0, HMMPRED_EINVAL = 1, HMMPRED_EUNSUPPORTED = 2, HMMPRED_EHIP = 3 };
enum hmmpred_dtype { HMMPRED_F32 = 0, HMMPRED_F64 = 1 };

int hmmpred_abi_version(void);
const char* hmmpred_last_error(void);

/* Doubles of scratch of a call with n_rows rows, for every permitted chunk_len (-1 for bad arguments; D does not enter
 * today and is checked only). */
int64_t hmmpred_scratch_len(int K, int D, int64_t n_rows);

/* ln p_t of the n_rows rows x[n_rows][D] (x_dtype, row stride ldx >= D elements, read where they lie under stmix_logpdf's
 * alignment rule).
 *   pivot_dev [D], img_dev      as given to stmix_pack (K components of D dimensions)
 *   c_dev, nu_dev [K]           c_k and nu_k
 *   a_dev [K][K], w0_dev [K]    transition matrix (row-major) and the first row's state distribution
 *   chunk_len, sweep_len        steps per chunk (0, or HMMPRED_MIN_CHUNK .. ) and steps walked in front of a boundary
 *                               (0, or 1 .. ; at most a chunk is walked); 0 = the defaults: one serial walk below 4096
 *                               rows, chunks of 32 up to 32768 rows, chunks of 256 beyond, 64 steps swept
 *   scratch_dev                 hmmpred_scratch_len(K, D, n_rows) doubles, 16-byte aligned
 *   lnp_dev [n_rows]            ln p_t
 *   z_dev [n_rows] int64        z_t; may be NULL
 *   end_dev [K]                 phi_{n_rows - 1}, natural state order
 *   diag_dev [2] int64          chunks whose start vector did not stand; chunks walked again */
int hmmpred_logpdf(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* pivot_dev,
                   const double* img_dev, const double* c_dev, const double* nu_dev, const double* a_dev,
                   const double* w0_dev, int64_t chunk_len, int64_t sweep_len, double* scratch_dev, double* lnp_dev,
                   int64_t* z_dev, double* end_dev, int64_t* diag_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMMPRED_H */
