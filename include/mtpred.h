/*
 * mtpred.h — C ABI of the meta-tree predictive log-density on the MI355X (gfx950), in libgmmvb.so beside mtree.h.
 *
 * mtree_predict (mtree.h) folds node values that do not depend on a label.  The predictive density of LABELLED rows does:
 * under the fixed posterior forest,
 *     lnp[i] = ln sum_b prob_b value_b(i),
 *     value(v) = p_v(y_i | x_i) at the node where row i's walk in tree b stops,
 *     value(v) = (1 - g_v) p_v(y_i | x_i) + g_v value(child) above it,
 * with p_v the sub-model's posterior predictive at node v: Bernoulli, categorical, negative binomial (poisson), Lomax
 * (exponential), Student-t (normal) and the Student-t of a Bayesian linear regression on all continuous features
 * (linear regression; its precision depends on the row's x).  mtpred_logpdf evaluates this in the LOG domain in one pass, so
 * a far-tail label gives a finite lnp where the linear-domain fold underflows to a density of 0.
 *
 * The forest (struct mtree_forest), the element types (enum mtree_dtype), the families (enum mtree_family), the walk, the
 * layout of post_dev (mtree_stat_cols) and the limits (MTREE_MAX_*, MTREE_LR_MAX_DEGREE) are mtree.h's, and so are the
 * conventions: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed as void*
 * (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the return value is an
 * mtree_status code and mtpred_last_error() gives a thread-local message.  Arguments are validated before anything touches
 * the device, so bad arguments are reported without a GPU.  Every table index is range-checked on the device before use.
 * No floating-point atomics: two calls give the same bits.
 *
 * The pass.  A workgroup of MTPRED_WAVES waves owns a tile of MTPRED_TILE rows; a lane is a row and
 * wave w takes trees w, w + MTPRED_WAVES, ...  The tile's features (continuous widened to binary64, categorical as int32) and
 * labels are staged in LDS once and reused by every tree; a tile whose features exceed MTPRED_LDS_BYTES is read where it lies.
 * Per node and per call, constants are built from post_dev so that a visit evaluates nothing that does not depend on y.
 * A lane walks its tree (at most forest->max_depth levels), keeps the path, and folds from the stop node up:
 *     value = ln p_v                                                     at the stop node,
 *     value = max(a, c) + log1p(exp(-|a - c|)), a = ln(1 - g) + ln p_v, c = ln g + value(child)   above it;
 * g <= 0 takes ln p_v and g >= 1 the child's value bit for bit, two -inf give -inf.  A wave mixes its trees by a running
 * (max, scaled sum) log-sum-exp of ln prob_b + value_b in tree order (prob_b <= 0 is skipped), the wave partials are combined
 * through LDS in wave order, so the result does not depend on scheduling.
 *
 * Linear regression: a node's constants are a 16 x 16 operand image (row a < degree holds row a of the inverse Cholesky
 * factor W of Lambda, row 15 holds mu, zeros elsewhere) and four scalars.  At every level a wave ballots the distinct nodes
 * of its lanes; for a node shared by at least MTPRED_SHARE lanes the image times the tile's X' (16 x 64, x padded to 16) on
 * v_mfma_f64_16x16x4_f64 gives W x and mu . x of all 64 rows at once and the node's lanes take their column; the other
 * lanes evaluate the triangular form themselves.  Both paths give the same value up to the order of their sums, so for this
 * family a row's lnp may depend on which rows share its tile; for the five scalar families it does not.
 */
#ifndef MTPRED_H
#define MTPRED_H

#include <stdint.h>

#include "mtree.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTPRED_ABI_VERSION 1
#define MTPRED_TILE 64
#define MTPRED_WAVES 4
/* the staged features of one tile, MTPRED_TILE * (8 dim_cont + 4 dim_cat) bytes, stay below this */
#define MTPRED_LDS_BYTES 32768
/* linear regression: lanes of a wave that must share a node for the node to go to the matrix pipe (1 = always, 65 = never).
 * A compile-time constant: -DMTPRED_SHARE=<k> builds a variant library for measurements (tools/bench_mtpred.py). */
#ifndef MTPRED_SHARE
#define MTPRED_SHARE 16
#endif
/* doubles per node of a linear-regression node's constants: the 16 x 16 image and
 * [ (alpha / beta) / nu, (nu + 1) / 2, lgamma((nu + 1) / 2) - lgamma(nu / 2) + ln((alpha / beta) / (pi nu)) / 2, nu ] */
#define MTPRED_LR_CONSTS 260

int mtpred_abi_version(void);
const char* mtpred_last_error(void);

/* 8-byte slots of consts_dev; -1 on bad arguments.  Per node:
 *   bernoulli    [ ln(alpha / (alpha + beta)), ln(beta / (alpha + beta)) ]                  (y = 1, y = 0)
 *   categorical  [ ln(alpha_a / sum alpha) ], degree entries
 *   poisson      [ lgamma(alpha), alpha ln(beta / (1 + beta)), ln(1 + beta) ]               (negative binomial)
 *   exponential  [ ln alpha + alpha ln beta, alpha + 1, beta ]                               (Lomax)
 *   normal       [ m, lambda / nu, (nu + 1) / 2, lgamma((nu + 1) / 2) - lgamma(nu / 2) + ln(lambda / (pi nu)) / 2 ],
 *                lambda = kappa / (kappa + 1) alpha / beta, nu = 2 alpha
 *   linreg       MTPRED_LR_CONSTS entries, above */
int64_t mtpred_consts_len(int32_t n_nodes, int family, int degree);
/* 8-byte slots of work_dev for n rows: one per tile when `total` is non-zero, else 0; -1 on bad arguments. */
int64_t mtpred_work_len(int64_t n, int total);

/* lnp_dev[i], i < n.  xc_dev, xk_dev: the rows as mtree_route takes them; y_dev: n labels, int64 for bernoulli /
 * categorical / poisson, binary64 otherwise; a label outside the family's support (not 0 / 1, a class outside
 * 0..degree-1, a negative count or waiting time) gives -inf.  post_dev[n_nodes][n_post], g_dev[n_nodes], prob_dev[n_trees]:
 * the posterior tables, read only.  consts_dev: mtpred_consts_len slots, overwritten.  total_dev: NULL, or one double that
 * receives sum_i lnp[i]: per-tile sums (a fixed lane butterfly) go to work_dev (mtpred_work_len slots) and one workgroup adds
 * them on a fixed tree.  Linear regression needs degree == forest->dim_cont. */
int mtpred_logpdf(const mtree_forest* forest, int family, int degree, int xc_dtype, const void* xc_dev, int xk_dtype,
                  const void* xk_dev, const void* y_dev, int64_t n, const double* post_dev, const double* g_dev,
                  const double* prob_dev, double* consts_dev, double* lnp_dev, double* total_dev, void* work_dev,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTPRED_H */
