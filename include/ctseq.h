/*
 * ctseq.h — C ABI of the sequential context-tree engine on the MI355X (gfx950), in libgmmvb.so beside ctree.h and ctsp.h.
 *
 * The reference (bayesml/BayesML v0.3.1, bayesml/contexttree/_contexttree.py:1016-1067) predicts symbol i from the
 * posterior of x[0..i-1] and then folds x[i] in, one call per symbol.  ctseq_pass does that for a whole run of positions
 * at once and returns every intermediate prediction; the posterior tables of ctree.h are left as the per-symbol loop
 * leaves them.  The level-wise form is DESIGN.md §4h, "Sequential prediction": per level, the visits of a node are brought
 * together in time order by a stable counting partition, the counts a visit sees are ranks, and a node's log-odds before a
 * visit are its starting log-odds plus a segmented prefix sum.
 *
 * Conventions are ctree.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the
 * return value is a status code (same values as enum ctree_status) and ctseq_last_error() gives a thread-local message.
 * Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * Tables and notation are ctree.h's (dense, all levels back to back).  No floating-point atomics, no device-side
 * recursion, no grid-wide waits; the scans run on fixed trees, so results are the same from run to run.  Every table
 * index is range-checked on the device before use.  The caller has validated the sample (ctree_count's bad = 0): a symbol
 * outside 0..k-1 is never used as an index, it is read as symbol 0, and what the call then computes means nothing.
 *
 * Limits: those of ctree.h (CTREE_MAX_K, CTREE_MAX_SLOTS), CTSEQ_EUNSUPPORTED beyond them.
 */
#ifndef CTSEQ_H
#define CTSEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTSEQ_ABI_VERSION 1
/* Positions per workgroup of the partitions and of the segmented scans (one per thread). */
#define CTSEQ_TILE 256
/* Visits that one lane group of the row pass walks in sequence. */
#define CTSEQ_ROW_BLOCK 64

enum ctseq_status { CTSEQ_OK = 0, CTSEQ_EINVAL = 1, CTSEQ_EUNSUPPORTED = 2, CTSEQ_EHIP = 3 };
enum ctseq_dtype { CTSEQ_U8 = 0, CTSEQ_I32 = 1, CTSEQ_I64 = 2 };

int ctseq_abi_version(void);
const char* ctseq_last_error(void);

/* 8-byte slots of scratch that ctseq_pass needs for m positions.  want_rows != 0: the scratch also holds an [m][k]
 * binary64 row buffer, at its start, which ctseq_pass needs and fills when argmax_dev is given without rows_dev.
 * -1 for k < 1, D < 1, m < 1, m >= 2^31 or a (k, D) beyond the limit. */
int64_t ctseq_work_len(int k, int D, int64_t m, int want_rows);

/* Positions begin .. begin + m - 1 of the sample x_dev[0..n-1] (`dtype`, aligned to the element size, read where it
 * lies): for each, the predictive distribution before the symbol is seen, then the update by it, in this order.  Contexts
 * are read from x[i - j] wherever i - j >= 0, so only a chunk with begin < D has positions that end above depth D.
 * State, all levels, updated in place: beta_dev[node][k] and g_dev[node] binary64, exists_dev[node] and leaf_dev[node]
 * uint8.  A node with exists = 0 reads hn_beta_dev[k] (device) and hn_g (0 at depth D); every visited node exists
 * afterwards, a new one at depth D with leaf = 1.  beta += the exact integer count of the chunk, in one addition.
 * Outputs, each may be NULL: rows_dev[m][k] binary64, the distributions; argmax_dev[m] int64, the first maximum of each;
 * nats_dev[m] binary64, -ln of the probability that the distribution of position i gave x[i]. */
int ctseq_pass(int dtype, const void* x_dev, int64_t n, int64_t begin, int64_t m, int k, int D, void* beta_dev, void* g_dev,
               void* exists_dev, void* leaf_dev, double hn_g, const void* hn_beta_dev, void* rows_dev, void* argmax_dev,
               void* nats_dev, void* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTSEQ_H */
