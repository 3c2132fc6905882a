/*
 * regseq.h — C ABI of sequential prediction for the Normal-Gamma regression family on the MI355X (gfx950), in
 * libgmmvb.so beside regvb.h.
 *
 * What n calls of LearnModel.pred_and_update do row by row (bayesml/linearregression/_linearregression.py:789-792,
 * bayesml/autoregressive/_autoregressive.py:692-698) - the Student-t predictive of row i from the posterior of the rows
 * before it, then the update by row i - in one group of launches per pass.  The rows of a call are cut into blocks; within a
 * block the predictive parameters come from the Cholesky factor of the block's marginal covariance, and the state at a
 * block's start is a function of the statistics [G | c | s | n] (regvb.h) of the rows before it (DESIGN.md 4f,
 * "Sequential prediction").
 *
 * The schedule of a call of n rows: blocks of 1, 2, 4, ..., REGSEQ_BLOCK / 2 rows (the leading ramp: a first block must
 * not see many rows through a diffuse prior), then blocks of REGSEQ_BLOCK rows, the last one cut at n.  It belongs to the
 * call, not to a pass: a pass is a range of whole blocks of it.
 *
 * Conventions are regvb.h's: *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed as void*; calls
 * only enqueue work, never allocate, never synchronise; the return value is a status code and regseq_last_error() gives a
 * thread-local message.  Arguments are validated before anything touches the device.  Rows stay in their storage dtype
 * (REGSEQ_F32 or REGSEQ_F64, regvb.h's codes) and are widened on load.  No sum uses atomics, no kernel waits for another workgroup: two
 * calls on the same input give the same bits, and so do one pass and several passes over the same blocks.
 */
#ifndef REGSEQ_H
#define REGSEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REGSEQ_ABI_VERSION 1
#define REGSEQ_MAX_DEGREE 256
#define REGSEQ_BLOCK 64

enum regseq_status { REGSEQ_OK = 0, REGSEQ_EINVAL = 1, REGSEQ_EUNSUPPORTED = 2, REGSEQ_EHIP = 3 };
enum regseq_dtype { REGSEQ_F32 = 0, REGSEQ_F64 = 1 };
enum regseq_padding { REGSEQ_PAD_NONE = 0, REGSEQ_PAD_ZEROS = 1 };

int regseq_abi_version(void);
const char* regseq_last_error(void);

/* The block length B for D features (-1 for D outside 1..256).  A compile-time function of D; this version answers
 * REGSEQ_BLOCK for every D: the B x B factorisation of a block and one slice of its rows share the CU's LDS. */
int regseq_block(int D);
/* Blocks of the schedule of n rows (-1 for n < 1), and the first row of block b, 0 <= b <= regseq_block_count(n)
 * (block_start(n, count) = n; -1 outside). */
int64_t regseq_block_count(int64_t n);
int64_t regseq_block_start(int64_t n, int64_t b);
/* Doubles of scratch a pass over `blocks` blocks of D features needs (-1 for bad arguments): the block table, one slab
 * of partial sums and one start state (D rounded up to 16, squared, doubles) per block. */
int64_t regseq_work_len(int D, int64_t blocks);

/* One pass over the rows [row_begin, row_begin + row_count) of the n_rows rows x[n_rows][D] (row stride ldx >= D) with
 * targets y[n_rows]; the range must be whole blocks of the schedule of n_rows.
 *   start_dev  [D*D + D + 3]  the state at row 0:  Lambda_0 [D][D] | Lambda_0 mu_0 [D] | mu_0^T Lambda_0 mu_0, alpha_0, beta_0
 *   carry_dev  [D*D + D + 2]  [G | c | s | n] of the rows before row_begin (zeros for row_begin = 0); on return, of the
 *                             rows before row_begin + row_count
 *   p_m_dev, p_lambda_dev, p_nu_dev, nats_dev  [n_rows] each, indexed by the row; only the pass's rows are written; any of
 *                             them may be NULL.  nats = -ln St(y_i | p_m, p_lambda, p_nu).
 *   work_dev   [regseq_work_len(D, blocks of the range)] */
int regseq_pass(int D, int x_dtype, const void* x_dev, int64_t ldx, int y_dtype, const void* y_dev, int64_t n_rows,
                int64_t row_begin, int64_t row_count, const double* start_dev, double* carry_dev, double* p_m_dev,
                double* p_lambda_dev, double* p_nu_dev, double* nats_dev, double* work_dev, void* stream);

/* The same for the lag windows of a series x[length] of degree p (D = p + 1), rows and padding as regvb_stats_window:
 * n_rows = length - p (REGSEQ_PAD_NONE) or length (REGSEQ_PAD_ZEROS); outputs are indexed by the row, not by the time. */
int regseq_pass_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding, int64_t row_begin,
                       int64_t row_count, const double* start_dev, double* carry_dev, double* p_m_dev,
                       double* p_lambda_dev, double* p_nu_dev, double* nats_dev, double* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REGSEQ_H */
