/*
 * stmix.h — C ABI of the Student-t mixture log-density on the MI355X (gfx950), in libgmmvb.so beside gmmvb.h.
 *
 * The predictive distribution of gaussianmixture (bayesml/gaussianmixture/_gaussianmixture.py:1064-1070) is a mixture of
 * multivariate Student-t components; multivariate_normal's (:705-711) is the same with one component.  For rows x_i
 *
 *     t_ik     = c_k - a_k log1p(q_ik / nu_k),   q_ik = || U_k (x_i - mu_k) ||^2,   a_k = (nu_k + D) / 2
 *     ln p_i   = logsumexp_k t_ik,               z_i = the first k that maximises t_ik
 *     c_k      = ln pi_k + lnGamma(a_k) - lnGamma(nu_k / 2) - (D / 2) ln(nu_k pi) + sum_j ln U_k[j][j]
 *
 * with U_k lower triangular, U_k^T U_k = Lambda_k the component's scale (precision) matrix.  One launch evaluates ln p
 * (and z) of every row: the quadratic forms of gmmvb_estep's dense kernel on the f64 matrix pipe, closed in registers by
 * the Student-t log-kernel and a running log-sum-exp over the components.  No [n_rows][K] array exists anywhere
 * ("Predictive log-density of a sample").
 *
 * The parameters travel as an image (stmix_pack): for D <= 128 the E-step's tiled image of U_k, for D > 128 U_k itself,
 * each with the bias -U_k (mu_k - pivot) behind it.  The kernels subtract the same `pivot` from a row while they widen it
 * to binary64, so a sample far from the origin is centred before anything is multiplied.  Any [D] vector near the rows
 * serves; it must be the same in stmix_pack and stmix_logpdf.
 *
 * Conventions are ctree.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the return
 * value is a status code (same values as enum gmmvb_status) and stmix_last_error() gives a thread-local message.
 * Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * No atomics, no dependence between rows: a row's results do not depend on n_rows, on the tile the row lands in or on the
 * grid, and two calls give the same bits.  Nothing past entry n_rows - 1 of an output is written.
 */
#ifndef STMIX_H
#define STMIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STMIX_ABI_VERSION 1
#define STMIX_MAX_DEGREE 19200 /* above 128 a plain f64 kernel: correct, far slower */
#define STMIX_MAX_COMPONENTS 65536

enum stmix_status { STMIX_OK = 0, STMIX_EINVAL = 1, STMIX_EUNSUPPORTED = 2, STMIX_EHIP = 3 };
enum stmix_dtype { STMIX_F32 = 0, STMIX_F64 = 1 };

int stmix_abi_version(void);
const char* stmix_last_error(void);

/* Doubles of the parameter image of K components of D dimensions (-1 for bad arguments). */
int64_t stmix_image_len(int K, int D);

/* u_dev [K][D][D] (row-major, lower triangular: entries above the diagonal are not read), m_dev [K][D], pivot_dev [D]
 * ->  img_dev [stmix_image_len(K, D)]. */
int stmix_pack(int K, int D, const double* u_dev, const double* m_dev, const double* pivot_dev, double* img_dev,
               void* stream);

/* ln p of the n_rows rows x[n_rows][D] (x_dtype, row stride ldx >= D elements, read where they lie: 4-element vector loads
 * when D is a multiple of 16 and base and stride are multiples of four elements, scalar loads otherwise - same bits).
 *   pivot_dev [D], img_dev   as given to stmix_pack
 *   c_dev, nu_dev [K]        c_k and nu_k (nu_k > 0)
 *   lnp_dev [n_rows]         ln p_i
 *   z_dev   [n_rows] int64   z_i; may be NULL */
int stmix_logpdf(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* pivot_dev,
                 const double* img_dev, const double* c_dev, const double* nu_dev, double* lnp_dev, int64_t* z_dev,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STMIX_H */
