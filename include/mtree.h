/*
 * mtree.h — C ABI of the meta-tree forest engine on the MI355X (gfx950), in libgmmvb.so beside gmmvb.h, regvb.h, expfam.h
 * and ctree.h.
 *
 * The reference (bayesml/BayesML v0.3.1, bayesml/metatree/_metatree.py) updates a forest of meta-trees by boolean-mask
 * recursion in Python, once per tree and once per node (:1729-1770), and predicts the same way (:3217-3310).  The batch
 * form is: route every row through every tree (mtree_route), reduce the rows' y to per-node
 * statistics without floating-point atomics (mtree_reduce), and sweep every tree bottom-up in one launch (mtree_sweep):
 * children's statistics into the parent, the family's conjugate fold, its log marginal likelihood, and the two-way
 * mixture that ctree.h's sweep applies.  mtree_predict folds the per-node predictive values along every row's path of
 * every tree and mixes the trees.
 *
 * MTREE_LINREG puts a Bayesian linear regression over ALL continuous features into every node (the reference's
 * SubModel=linearregression, :1772-1817 and :3239-3259), so a node's statistics are X'X, X'y, y'y and n of its rows.  Its
 * reduction needs x and has an entry point of its own, mtree_reduce_x: the rows of every tree are sorted stably by (stop node,
 * row index) with a counting sort, and a segmented Gram pass forms one Z'Z per node on v_mfma_f64_16x16x4_f64, Z = [X | y]
 * padded to 16 columns, which is why the degree is at most MTREE_LR_MAX_DEGREE (two-tile rows, up to degree 30, are not
 * built).  mtree_sweep and mtree_predict take the family as they stand; its predictive tables are sized by mtree_values_len.
 *
 * Conventions are ctree.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the return
 * value is a status code and mtree_last_error() gives a thread-local message.  Arguments are validated before anything
 * touches the device, so bad arguments are reported without a GPU.
 *
 * The forest: flat node tables over all trees.  tree_off[b] is the first node of tree b (tree_off[n_trees] = n_nodes); within a
 * tree the nodes are in breadth-first order, so a parent precedes its children and siblings are contiguous.  Per node:
 * feat (the feature an inner node splits on, -1 for a leaf; features 0..dim_cont-1 are continuous, the rest categorical),
 * child0 (table index of the first child), nchild, thr_off (a continuous inner node's nchild + 1 thresholds start at
 * thr[thr_off]; the walk reads thr[thr_off + 1 .. thr_off + nchild - 1]) and depth (0 at a root).
 *
 * The walk of a row starts at the root.  A continuous node sends it to child 0 if x < thr[1], to child C-1 if
 * thr[C-1] <= x, to child i if thr[i] <= x < thr[i+1]; a categorical node to child x.  A row that matches no child (NaN, a
 * categorical value outside 0..C-1) stops at that node.  Every table index is range-checked on the device before use and a
 * child index must be larger than its parent's and inside the tree, so a malformed table ends a walk instead of looping.
 *
 * Limits (the reference has none): MTREE_MAX_TREES trees, MTREE_MAX_NODES nodes per tree, MTREE_MAX_CHILDREN children per
 * node, MTREE_MAX_DEGREE classes of the categorical sub-model, MTREE_LR_MAX_DEGREE regressors of the linear-regression
 * sub-model, MTREE_MAX_DEPTH levels below a root.  Beyond them every entry point returns MTREE_EUNSUPPORTED.
 */
#ifndef MTREE_H
#define MTREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTREE_ABI_VERSION 2
#define MTREE_MAX_TREES 1024
#define MTREE_MAX_NODES 4096
#define MTREE_MAX_CHILDREN 16
#define MTREE_MAX_DEGREE 16
#define MTREE_MAX_DEPTH 24
#define MTREE_MAX_SLABS 64
/* A tree whose statistics table (nodes x columns) has at most this many 8-byte slots (48 KiB) is reduced in a wave-private
 * LDS table; a larger one in the wave's slab of global scratch. */
#define MTREE_LDS_SLOTS 6144
/* Linear regression: the largest degree (x and y share one 16-column MFMA tile), and the sorted positions one wave of the
 * segmented Gram pass owns (a node's sum is cut where its segment crosses a multiple of this, so it is part of the bits). */
#define MTREE_LR_MAX_DEGREE 15
#define MTREE_LR_BLOCK 1024

enum mtree_status { MTREE_OK = 0, MTREE_EINVAL = 1, MTREE_EUNSUPPORTED = 2, MTREE_EHIP = 3 };
enum mtree_dtype { MTREE_U8 = 0, MTREE_I32 = 1, MTREE_I64 = 2, MTREE_F32 = 3, MTREE_F64 = 4 };
enum mtree_family {
    MTREE_BERNOULLI = 0, MTREE_CATEGORICAL = 1, MTREE_POISSON = 2, MTREE_EXPONENTIAL = 3, MTREE_NORMAL = 4, MTREE_LINREG = 5
};
/* What mtree_predict writes per row: the mixed mean (one double), the mixed class probabilities (C doubles), their argmax
 * (one int64), or the mixed predictive variance (one double; normal and linear regression). */
enum mtree_pred { MTREE_PRED_MEAN = 0, MTREE_PRED_PROBA = 1, MTREE_PRED_CLASS = 2, MTREE_PRED_VAR = 3 };

typedef struct mtree_forest {
    int32_t n_trees, n_nodes, n_thr;        /* n_nodes, n_thr: entries of the node tables and of thr_dev, all trees */
    int32_t max_tree_nodes, max_children;   /* the largest tree and the widest node (checked against the limits) */
    int32_t max_depth;                      /* the deepest node's depth */
    int32_t dim_cont, dim_cat;
    const int32_t* tree_off_dev;            /* [n_trees + 1] */
    const int32_t* feat_dev;                /* [n_nodes] each */
    const int32_t* child0_dev;
    const int32_t* nchild_dev;
    const int32_t* thr_off_dev;
    const int32_t* depth_dev;
    const double* thr_dev;                  /* [n_thr] (may be NULL when n_thr = 0) */
} mtree_forest;

int mtree_abi_version(void);
const char* mtree_last_error(void);

/* Columns of the family's statistics: n_int int64 columns [ n | ... ] and n_real binary64 columns per node, and the length
 * n_post of its posterior vector:
 *   bernoulli    int [n, sum y]            real -                         post [alpha, beta]
 *   categorical  int [n, c_0..c_{deg-1}]   real -                         post [alpha_0..alpha_{deg-1}]
 *   poisson      int [n, sum y]            real [sum ln y!]               post [alpha, beta, sum ln y!]
 *   exponential  int [n]                   real [sum y]                   post [alpha, beta]
 *   normal       int [n]                   real [mu, c, SS]               post [m, kappa, alpha, beta, n]
 *   linreg       int [n]                   real [ut(X'X), X'y, y'y]       post [mu_0..mu_{deg-1}, ut(Lambda), alpha, beta, n]
 * ut(.) is the upper triangle, row-major, deg (deg + 1) / 2 entries.  Returns 0, or MTREE_EINVAL / MTREE_EUNSUPPORTED for an
 * unknown family or a degree outside 1..MTREE_MAX_DEGREE (categorical) or 1..MTREE_LR_MAX_DEGREE (linreg). */
int mtree_stat_cols(int family, int degree, int* n_int, int* n_real, int* n_post);
/* 8-byte slots of scratch for mtree_reduce and mtree_sweep with n_slabs slabs (one buffer serves both); -1 on bad arguments. */
int64_t mtree_work_len(int32_t n_nodes, int family, int degree, int n_slabs);

/* stop_dev[b * n + i] = the node where row i's walk in tree b stops.  xc_dev: [n][dim_cont] of xc_dtype (F32 or F64), xk_dev:
 * [n][dim_cat] of xk_dtype (U8, I32 or I64), row-major, read where they lie (NULL where the dimension is 0).  cat_card_dev:
 * [dim_cat] int32, the number of values of every categorical feature; bad_dev[0] is set to the number of categorical entries
 * outside 0..cat_card-1 (they are never used as an index).  path_dev: NULL, or int32 [n_trees][n][max_depth + 1]: the nodes of
 * the walk, root first, padded with -1. */
int mtree_route(const mtree_forest* f, int xc_dtype, const void* xc_dev, int xk_dtype, const void* xk_dev,
                const int32_t* cat_card_dev, int64_t n, int32_t* stop_dev, int32_t* path_dev, int64_t* bad_dev, void* stream);

/* Per (tree, stop node), the statistics of the y of the rows that stop there, into stat_int_dev[n_nodes][n_int] and
 * stat_real_dev[n_nodes][n_real] (overwritten).  y_dev: n values, int64 for bernoulli / categorical / poisson, binary64 for
 * exponential / normal; a value outside the family's support is left out of every column but n.  Integer columns are
 * integer atomics (exact, order-free).  Real columns use no floating-point atomics and are bit-reproducible: a wave owns a
 * contiguous slab of rows of one tree and a table only it writes, adds the lanes that share a node in fixed lane order, and
 * the slabs are added in slab order.  Normal takes two passes and no pivot that nodes would share: the first sums y per stop
 * node, the second sums r = y - mu and r^2 about the node's own mu = (sum y) / n, and leaves [sum y, sum r, sum r^2]. */
int mtree_reduce(const mtree_forest* f, int family, int degree, const int32_t* stop_dev, const void* y_dev, int64_t n,
                 int n_slabs, int64_t* stat_int_dev, double* stat_real_dev, void* work_dev, void* stream);

/* 8-byte slots of scratch for mtree_reduce_x on n rows with n_slabs slabs: the slab histograms, the segment starts, every
 * tree's sorted row indices and the boundary slots of the Gram pass; -1 on bad arguments. */
int64_t mtree_reduce_x_work_len(int32_t n_nodes, int32_t n_trees, int degree, int64_t n, int n_slabs);
/* mtree_reduce for a family whose statistics need x (MTREE_LINREG; any other family is MTREE_EINVAL, it has mtree_reduce).
 * x_dev: n rows of `degree` regressors of x_dtype (F32 or F64), `x_stride` elements from one row to the next
 * (x_stride >= degree), read where they lie and widened to binary64; y_dev: n binary64 values; n < 2^31.  Per tree the row
 * indices are sorted stably by (stop node, row index): per-slab node histograms (integer atomics), a scan, and a scatter in
 * which every slab writes its rows in row order, so the order does not depend on how atomics land.  The sorted array is cut
 * into blocks of MTREE_LR_BLOCK positions; a wave adds its block's rows four at a time, run by run (a run = one node's
 * positions), runs inside a block go straight to the node, the block's first and last run to boundary slots that a last
 * pass adds in block order.  n is the segment's length, exact.  No floating-point atomics: two calls give the same bits.
 * A row whose stop node is outside its tree is left out. */
int mtree_reduce_x(const mtree_forest* f, int family, int degree, const int32_t* stop_dev, int x_dtype, const void* x_dev,
                   int64_t x_stride, const double* y_dev, int64_t n, int n_slabs, int64_t* stat_int_dev,
                   double* stat_real_dev, void* work_dev, void* stream);

/* One launch, a workgroup per tree, depth by depth from the deepest to the root.  In place: the statistics become subtree
 * totals (children added in child order).  A normal node carries [mu, c, SS]: its mean is mu + c / n, formed once, at the
 * fold, and SS is about that mean; the parts of a node (its own rows, its children) merge about mu_P = their rounded common
 * mean, c_P = sum [c_i + n_i (mu_i - mu_P)], SS_P = sum [SS_i + n_i dm_i^2], dm_i = (mu_i - mu_P) + (c_i / n_i - c_P / n_P).
 * A node with n = 0 is left
 * bit-identical and its parent takes 0.0 for it; every other node gets its posterior folded (post_dev[n_nodes][n_post]),
 * lml_dev[node] = the family's log marginal likelihood of the folded posterior against h0_dev[n_post], and an inner node
 * g <- exp(t1 - L), t1 = ln g + sum of the children's L, L = logaddexp(ln(1 - g) + lml, t1); g = 0 and g = 1 are fixed
 * points.  lcm_dev[c] = the L (0.0 for an empty child) that the visited parent of node c took for it, the reference's
 * log_children_marginal_likelihood.  lnp_dev[b] += L of the root. */
int mtree_sweep(const mtree_forest* f, int family, int degree, int64_t* stat_int_dev, double* stat_real_dev,
                const double* h0_dev, double* post_dev, double* g_dev, double* lml_dev, double* lcm_dev, double* lnp_dev,
                void* work_dev, void* stream);

/* 8-byte slots of mtree_predict's values_dev for any mode: n_nodes * max(2, degree), and for linear regression
 * n_nodes * (degree + degree (degree + 1) / 2 + 2); -1 on bad arguments. */
int64_t mtree_values_len(int32_t n_nodes, int family, int degree);

/* values_dev[n_nodes][C] is filled from the posteriors (per node, once per call), then every row's walk in every tree is
 * folded bottom-up, value(v) = (1 - g_v) p_v + g_v value(child), p_stop at the node where the walk stops, and the trees are
 * mixed with prob_dev[n_trees].  C = 1 for MEAN and VAR (VAR uses two tables of C = 1: values_dev holds 2 n_nodes doubles),
 * 2 for bernoulli and `degree` for categorical with PROBA / CLASS.  out_dev: binary64 [n] (MEAN, VAR), [n][C] (PROBA) or
 * int64 [n] (CLASS).  A family that has no such read-out (MEAN on a classifier, PROBA / CLASS on a regressor, VAR on anything
 * but normal and linear regression) is MTREE_EINVAL.
 * Linear regression (degree must equal dim_cont): values_dev holds mtree_values_len slots, per node [mu | the packed inverse
 * Cholesky factor W of Lambda | alpha / beta | 2 alpha]; at every node of a row's walk p_v(x) = x . mu_v and, for VAR,
 * nu / lambda / (nu - 2) with lambda = (alpha / beta) / (1 + |W x|^2), NaN when nu <= 2. */
int mtree_predict(const mtree_forest* f, int family, int degree, int mode, int xc_dtype, const void* xc_dev, int xk_dtype,
                  const void* xk_dev, int64_t n, const double* post_dev, const double* g_dev, const double* prob_dev,
                  double* values_dev, void* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTREE_H */
