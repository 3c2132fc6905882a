/*
 * mvnseq.h — C ABI of sequential prediction for the Gauss-Wishart model of multivariate_normal on the MI355X (gfx950), in
 * libgmmvb.so beside regseq.h.
 *
 * What n calls of LearnModel.pred_and_update do row by row (bayesml/multivariate_normal/_multivariatenormal.py:753-759) -
 * the multivariate Student-t predictive of row i from the posterior of the rows before it, then the update by row i - in
 * one group of launches per pass.  With S = hn_w_mat_inv and the innovation u_i = sqrt(kappa_i / (kappa_i + 1)) (x_i - m_i),
 * S_{i+1} = S_i + u_i u_i^T: the block structure of regseq.h with the innovation rows in the place of the regressors
 * ("Sequential prediction, multivariate normal").
 *
 * The schedule of a call of n rows is regseq.h's: blocks of 1, 2, 4, ..., MVNSEQ_BLOCK / 2 rows, then blocks of
 * MVNSEQ_BLOCK rows, the last one cut at n.  It belongs to the call, not to a pass: a pass is a range of whole blocks of it.
 *
 * Conventions are regseq.h's: *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed as void*;
 * calls only enqueue work, never allocate, never synchronise; the return value is a status code and mvnseq_last_error()
 * gives a thread-local message.  Arguments are validated before anything touches the device.  Rows stay in their storage
 * dtype (MVNSEQ_F32 or MVNSEQ_F64) and are widened on load.  No sum uses atomics, no kernel waits for another workgroup:
 * two calls on the same input give the same bits, and so do one pass and several passes over the same blocks.
 */
#ifndef MVNSEQ_H
#define MVNSEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVNSEQ_ABI_VERSION 1
#define MVNSEQ_MAX_DEGREE 256
#define MVNSEQ_BLOCK 64

enum mvnseq_status { MVNSEQ_OK = 0, MVNSEQ_EINVAL = 1, MVNSEQ_EUNSUPPORTED = 2, MVNSEQ_EHIP = 3 };
enum mvnseq_dtype { MVNSEQ_F32 = 0, MVNSEQ_F64 = 1 };

int mvnseq_abi_version(void);
const char* mvnseq_last_error(void);

/* The block length for D dimensions (-1 for D outside 1..256); this version answers MVNSEQ_BLOCK for every D. */
int mvnseq_block(int D);
/* Blocks of the schedule of n rows (-1 for n < 1), and the first row of block b, 0 <= b <= mvnseq_block_count(n)
 * (block_start(n, count) = n; -1 outside). */
int64_t mvnseq_block_count(int64_t n);
int64_t mvnseq_block_start(int64_t n, int64_t b);
/* Doubles of scratch a pass over `blocks` blocks of D dimensions needs (-1 for bad arguments): the block table and, per
 * block, the column sums, 64 rows of pivot-relative means and their scales, one slab of partial sums and one start
 * state (D rounded up to 16, squared, doubles). */
int64_t mvnseq_work_len(int D, int64_t blocks);

/* One pass over the rows [row_begin, row_begin + row_count) of the n_rows rows x[n_rows][D] (row stride ldx >= D); the
 * range must be whole blocks of the schedule of n_rows.
 *   start_dev  [D*D + D + 2]  the state at row 0:  S_0 = hn_w_mat_inv [D][D] | m_0 [D] | kappa_0, nu_0
 *   carry_dev  [D*D + D + 1]  [G | sum (x - pivot) | n] of the rows before row_begin, G the Gram matrix of their innovation
 *                             rows and pivot row 0 of x (zeros for row_begin = 0); on return, of the rows before
 *                             row_begin + row_count
 *   p_m_dev    [n_rows][D], row stride ld_pm >= D: the predictive mean of every row of the pass
 *   logdet_dev, quad_dev, nats_dev  [n_rows] each, indexed by the row: ln det p_v_mat, (x - p_m)^T p_v_mat (x - p_m) and
 *                             -ln St(x_i | p_m, p_v_mat, p_nu); only the pass's rows are written
 *   Any of the four outputs may be NULL.
 *   work_dev   [mvnseq_work_len(D, blocks of the range)] */
int mvnseq_pass(int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, int64_t row_begin, int64_t row_count,
                const double* start_dev, double* carry_dev, double* p_m_dev, int64_t ld_pm, double* logdet_dev,
                double* quad_dev, double* nats_dev, double* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVNSEQ_H */
