/*
 * hmmbatch.h — C ABI of the predictive log-density of MANY independent sequences under one hidden Markov model with
 * Student-t emissions on the MI355X (gfx950), in libgmmvb.so beside hmmpred.h.
 *
 * The model and the per-row quantities are hmmpred.h's: ln e_tk, m_t, rho'_tk, and for every sequence n with rows
 * off[n] .. off[n + 1] - 1 of x, on its own and from its own start vector w0_n,
 *
 *     w_t = phi_{t-1} A (t >= 1), w_0 = w0_n,   s_t = sum_k w_tk rho'_tk,   ln p_t = ln s_t + m_t,
 *     phi_t = s_t > 0 ? w_t o rho'_t / s_t : 0,   z_t = the first k that maximises phi_tk.
 *
 * The emission of all n_rows rows is hmmpred.h's (rows are independent: sequence boundaries do not enter).  The recursion
 * steps sixteen sequences at a time as the sixteen columns of v_mfma_f64_16x16x4_f64 up to 64 states - a sequence start is
 * an exact boundary, nothing is swept and nothing is gated - and runs as one serial walk per sequence for 65 .. 256 states
 * ("Predictive log-density of many sequences").  No [n_rows][K] array of phi exists.
 *
 * Conventions are hmmpred.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never synchronise; the return value is
 * a status code and hmmbatch_last_error() gives a thread-local message.  Arguments are validated before anything touches
 * the device, so bad arguments are reported without a GPU.  What lies in device memory cannot be: that off_dev ascends
 * from 0 to n_rows and that order_dev is a permutation of 0 .. n_seq - 1 is the caller's contract.
 *
 * No atomics; two calls give the same bits, and what a sequence gets depends on no other sequence of the batch nor on its
 * place in it.  Nothing is written outside lnp [n_rows], z [n_rows], end [n_seq][K] and tot [n_seq].
 */
#ifndef HMMBATCH_H
#define HMMBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMMBATCH_ABI_VERSION 1
#define HMMBATCH_MAX_DEGREE 19200 /* hmmpred.h's */
#define HMMBATCH_MAX_STATES 256   /* 1 .. 64 sixteen sequences per wave on the matrix pipe, 65 .. 256 a workgroup each */
#define HMMBATCH_MFMA_STATES 64
#define HMMBATCH_SHEAF 16         /* sequences a wave steps together */

enum hmmbatch_status { HMMBATCH_OK = 0, HMMBATCH_EINVAL = 1, HMMBATCH_EUNSUPPORTED = 2, HMMBATCH_EHIP = 3 };
enum hmmbatch_dtype { HMMBATCH_F32 = 0, HMMBATCH_F64 = 1 };

int hmmbatch_abi_version(void);
const char* hmmbatch_last_error(void);

/* Doubles of scratch of a call: rho' [npad][Kp] and m [npad] of the rows and the emission's ln e [K][npad], npad = n_rows
 * rounded up to 64, Kp = K rounded up to 16 (-1 for bad arguments; D and n_seq do not enter today and are checked only). */
int64_t hmmbatch_scratch_len(int K, int D, int64_t n_rows, int64_t n_seq);

/* ln p_t of the rows of n_seq >= 1 sequences laid end to end in x[n_rows][D] (x_dtype, row stride ldx >= D elements, read
 * where they lie under stmix_logpdf's alignment rule); n_rows >= 0.
 *   off_dev [n_seq + 1] int64   ascending row offsets, off[0] = 0, off[n_seq] = n_rows; equal neighbours = an empty sequence
 *   order_dev [n_seq] int32     the sequences in the order the kernel takes them up; any permutation gives the same bits,
 *                               longest first keeps the members of a wave alike and starts the long waves first
 *   pivot_dev [D], img_dev      as given to stmix_pack (K components of D dimensions)
 *   c_dev, nu_dev [K]           c_k and nu_k
 *   a_dev [K][K]                transition matrix (row-major)
 *   w0_dev, w0_stride           start vectors: stride 0 = one [K] vector for every sequence, stride K = [n_seq][K]
 *   scratch_dev                 hmmbatch_scratch_len(K, D, n_rows, n_seq) doubles, 16-byte aligned (unused for n_rows = 0)
 *   lnp_dev [n_rows]            ln p_t
 *   z_dev [n_rows] int64        z_t; may be NULL
 *   end_dev [n_seq][K]          the last phi of every sequence, natural state order; its start vector if it is empty
 *   tot_dev [n_seq]             sum of ln p_t over each sequence (hmmbatch_totals), 0.0 if empty; may be NULL */
int hmmbatch_logpdf(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, int64_t n_seq,
                    const int64_t* off_dev, const int32_t* order_dev, const double* pivot_dev, const double* img_dev,
                    const double* c_dev, const double* nu_dev, const double* a_dev, const double* w0_dev, int64_t w0_stride,
                    double* scratch_dev, double* lnp_dev, int64_t* z_dev, double* end_dev, double* tot_dev, void* stream);

/* tot[n] = sum of lnp[off[n] .. off[n + 1]) in a fixed order (a wave per sequence: 64 strided partial sums, then a
 * butterfly), 0.0 for an empty sequence; -inf propagates.  The same kernel closes hmmbatch_logpdf. */
int hmmbatch_totals(int64_t n_seq, const int64_t* off_dev, const double* lnp_dev, double* tot_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMMBATCH_H */
