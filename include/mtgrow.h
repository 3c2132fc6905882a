/*
 * mtgrow.h — C ABI of the level-synchronous growth engine behind metatree's MTMCMC / REMTMCMC on the MI355X (gfx950), in
 * libgmmvb.so beside mtree.h.
 *
 * The reference (bayesml/BayesML v0.3.1, bayesml/metatree/_metatree.py:2258-2436) proposes a tree by boolean-mask recursion
 * over all rows, node by node.  Here the proposals of all chains grow together, one level per mtgrow_level call, in tables
 * that mtree.h's mtree_forest describes, so mtree_route / mtree_reduce / mtree_reduce_x / mtree_sweep score them as they
 * stand; mtgrow_accept then applies the Metropolis-Hastings test per chain.
 *
 * Layout: every chain owns a complete C-ary tree of `cap` slots in heap order: the children of slot h are C h + 1 .. C h + C,
 * table index b * cap + h, a node's C + 1 thresholds at (b * cap + h) * (C + 1).  The static tables of the mtree_forest
 * (tree_off, child0, nchild, thr_off, depth) are the caller's; growth writes feat, thr, g and post only.
 *
 * Random numbers are addressed: draws_dev[b][h][0] is node h's keep / flip draw, draws_dev[b][h][1] its feature draw
 * (floor(u F), or floor(u (F - 1)) mapped past the excluded feature), so no draw's position depends on the data.
 *
 * Conventions are mtree.h's: *_dev pointers are DEVICE pointers owned by the caller, `stream` is a hipStream_t as void*; calls
 * only enqueue, never allocate, never synchronise; arguments are validated before anything touches the device.  No
 * floating-point atomics anywhere: integer atomics (exact, order-free) and fixed-order block scans, so two runs give the
 * same bits.
 */
#ifndef MTGROW_H
#define MTGROW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTGROW_ABI_VERSION 1
/* threads of the per-node 2-means workgroup: the sorted positions are taken this many at a time */
#define MTGROW_KMEANS_BLOCK 1024

enum mtgrow_status { MTGROW_OK = 0, MTGROW_EINVAL = 1, MTGROW_EUNSUPPORTED = 2, MTGROW_EHIP = 3 };
/* how a continuous split's thresholds are formed where lo < hi: arange(lo, hi + w / 2, w) with w = (hi - lo) / C, filled as
 * NumPy fills it (lo + i ((lo + w) - lo)); or, for C = 2 only, the midpoint between the two adjacent unique values that
 * minimises the 2-means cost (first index on ties). */
enum mtgrow_threshold { MTGROW_MIDPOINT = 0, MTGROW_KMEANS = 1 };

typedef struct mtgrow_state {
    int32_t n_chains, cap, n_children;   /* B, slots per chain, C; cap = (C^(max_depth + 1) - 1) / (C - 1) */
    int32_t dim_cont, dim_cat, max_depth, n_post, threshold;
    int64_t n;                           /* rows, 1 .. 2^31 - 1 */
    int32_t xc_dtype, xk_dtype;          /* enum mtree_dtype: F32 / F64, and U8 / I32 / I64 */
    const void* xc_dev;                  /* [n][dim_cont] (NULL where dim_cont = 0) */
    const void* xk_dev;                  /* [n][dim_cat] */
    const int32_t* order_dev;            /* [dim_cont][n]: the rows in ascending order of each continuous feature, NaN last
                                            (MTGROW_KMEANS only, else may be NULL) */
    const double* draws_dev;             /* [B][cap][2], in [0, 1) */
    const int32_t* last_feat_dev;        /* [B * cap] the chains' last trees */
    const double* last_g_dev;            /* [B * cap] */
    int32_t* feat_dev;                   /* [B * cap] the proposals: -1 for a leaf or a slot no row reaches */
    double* thr_dev;                     /* [B * cap * (C + 1)] */
    double* g_dev;                       /* [B * cap] */
    double* post_dev;                    /* [B * cap][n_post] */
    int32_t* node_dev;                   /* [B][n] the slot every row has reached */
    /* [B * cap] each: open (the parent split), regen (below a flip), dflag (0 not visited, 1 kept, 2 flipped), the lowest
       row index, the row count, "some row differs from the first", the encoded min and max of the split feature, the
       2-means threshold */
    int32_t *open_dev, *regen_dev, *dflag_dev, *first_dev, *count_dev, *differs_dev;
    uint64_t *lo_dev, *hi_dev;
    double* mid_dev;
} mtgrow_state;

int mtgrow_abi_version(void);
const char* mtgrow_last_error(void);

/* The slots of a complete C-ary tree of the given depth, or -1 where it exceeds MTREE_MAX_NODES or an argument is bad. */
int64_t mtgrow_capacity(int n_children, int max_depth);

/* Resets the proposals: feat = -1, the root open, every row at slot 0, g = g_root at slot 0, g_below at the other slots and
 * 0 at depth max_depth, post = sub_hn_dev[n_post] everywhere. */
int mtgrow_begin(const mtgrow_state* s, double g_root, double g_below, const double* sub_hn_dev, void* stream);

/* Grows level `level` (0 .. max_depth - 1) of every chain: the per-node decisions (a node below a flip, or every node when
 * all_regen != 0, draws its feature from all F; otherwise it keeps the last tree's unless u > min(last g, g_max)), the lowest
 * row and the count per node, the allclose test against the node's first row (|a - b| <= 1e-8 + 1e-5 |b|) and the exact min /
 * max of the split feature, the 2-means threshold where asked for, the leaf rule and the thresholds, and the rows' move to
 * their children by mtree_route's rule (a NaN, or a categorical value outside 0 .. C - 1, stays).  A child no row reaches
 * stays a leaf with n = 0. */
int mtgrow_level(const mtgrow_state* s, int level, int all_regen, double g_max, void* stream);

/* After mtree_sweep.  Per chain b: tp_x = sum over the kept nodes of ln min(g_x, g_max) + ln(1 - min(g_x, g_max)) at the
 * flipped node, for x = the proposal and the last tree; the proposal is accepted when
 *   u_dev[b] < exp((l_new - l_last) beta_dev[b] - tp_last + tp_new)     (tempered != 0), or
 *   u_dev[b] < exp(l_new - tp_last - l_last + tp_new)                   (tempered == 0),
 * and then feat, thr, g and post of the proposal, and the lml_dev / lcm_dev [B * cap] that mtree_sweep wrote for it, are
 * copied over the last tree's (last_*_dev, written here) and l_last_dev[b] = l_new.
 * out_dev[b][4] = { accepted, l_new, tp_new, tp_last }. */
int mtgrow_accept(const mtgrow_state* s, int tempered, double g_max, const double* l_new_dev, double* l_last_dev,
                  const double* beta_dev, const double* u_dev, const double* lml_dev, const double* lcm_dev,
                  int32_t* last_feat_dev, double* last_thr_dev, double* last_g_dev, double* last_post_dev,
                  double* last_lml_dev, double* last_lcm_dev, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGROW_H */
