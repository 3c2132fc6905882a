/*
 * ctree.h — C ABI of the context-tree engine on the MI355X (gfx950), in libgmmvb.so beside gmmvb.h, regvb.h and expfam.h.
 *
 * The reference (bayesml/BayesML v0.3.1, bayesml/contexttree/_contexttree.py) walks a Python node tree once per symbol
 * (:688-731).  The sequential update has a closed batch form ("Context tree"): count every (context, symbol)
 * pair at the deepest level, derive the upper levels' counts by child sums, and apply one Dirichlet-multinomial ratio
 * and one two-way mixture per node, bottom-up.  The entry points below are that count and that sweep, and the bottom-up
 * MAP sweep of :744-768.
 *
 * Conventions are expfam.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the
 * return value is a status code (same values as enum gmmvb_status) and ctree_last_error() gives a thread-local message.
 * Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * Notation: k symbols, maximal depth D, samples x[0..n-1].  A node at depth d is the context (x[i-1], ..., x[i-d]); its
 * key is  sum_{j=1..d} x[i-j] k^(j-1),  so level d has k^d keys and child c of key s has key  s + c k^d  at level d + 1.
 * A "level table" holds one entry per key of a level, keys in order; "all levels" means levels 0..D back to back, level
 * d starting at entry (k^d - 1) / (k - 1)  (d for k = 1).
 *
 * No floating-point atomics, no device-side recursion, no grid-wide waits: counts are 64-bit integers (exact and
 * order-free), the sweeps are one launch per level.  Every table index is range-checked on the device before use, and a
 * symbol outside 0..k-1 is never used as an index.
 *
 * Limit: k <= CTREE_MAX_K and k^(D+1) <= CTREE_MAX_SLOTS (the deepest count table).  Beyond it every entry point returns
 * CTREE_EUNSUPPORTED (k = 1: D <= 24).  The reference has no such limit.
 * (ctsp.h is the same update on sparse per-level hash tables, for shapes beyond this limit.)
 */
#ifndef CTREE_H
#define CTREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTREE_ABI_VERSION 1
#define CTREE_MAX_K 256
#define CTREE_MAX_SLOTS (1 << 24)
/* Deepest count tables of up to this many int64 bins (32 KiB) are counted in workgroup-private LDS histograms, one slab
 * per workgroup; larger ones by 64-bit integer global atomics into the zeroed table. */
#define CTREE_LDS_BINS 4096

enum ctree_status { CTREE_OK = 0, CTREE_EINVAL = 1, CTREE_EUNSUPPORTED = 2, CTREE_EHIP = 3 };
enum ctree_dtype { CTREE_U8 = 0, CTREE_I32 = 1, CTREE_I64 = 2 };

int ctree_abi_version(void);
const char* ctree_last_error(void);

/* Entries of level `level`'s table, k^level (0 <= level <= D);  with level = -1 the entries of all levels together.
 * -1 for k < 1, D < 1, a level outside -1..D, or a (k, D) beyond the limit. */
int64_t ctree_table_len(int k, int D, int level);
/* 8-byte slots of scratch that ctree_count, ctree_sweep and ctree_map need (one buffer serves all three); -1 as above. */
int64_t ctree_work_len(int k, int D);

/* Counts of the deepest level.  x_dev: n >= 1 symbols of `dtype`, aligned to the element size, read where they lie.
 * out_dev: 2 + k^(D+1) int64 slots  [ n | bad | cnt_D[k^D][k] ],  cnt_D[s][a] = number of i >= D with context key s and
 * x[i] = a.  `bad` counts the values outside 0..k-1; a sample i with a bad value anywhere in x[i-D..i] is not counted. */
int ctree_count(int dtype, const void* x_dev, int64_t n, int k, int D, void* out_dev, void* work_dev, void* stream);

/* The up-sweep, in place.  cnt_dev: the k^(D+1) counts of ctree_count (out_dev + 2 slots).  head_dev: the first
 * n_head = min(n, D) symbols of the sample as int32 (may be NULL when n_head = 0); sample d < n_head is the one that the
 * reference handles as a leaf at depth d.  State, all levels: beta_dev[node][k] and g_dev[node] binary64, exists_dev[node]
 * uint8.  A node with exists = 0 reads hn_beta_dev[k] (device) for its beta and hn_g (0 at depth D) for its g.  A node whose
 * count row sums to zero is left bit-identical; every other node gets beta += cnt, its new g, and exists = 1.
 * cnt_levels_dev: NULL, or int64 [nodes of levels 0..D-1][k]: the counts of the upper levels, for tests. */
int ctree_sweep(int k, int D, const void* cnt_dev, const void* head_dev, int n_head, void* beta_dev, void* g_dev,
                void* exists_dev, double hn_g, const void* hn_beta_dev, void* cnt_levels_dev, void* work_dev, void* stream);

/* The bottom-up MAP sweep of :744-768.  map_leaf_dev: uint8, all levels.  An existing node compares 1 - g with g times
 * the product of its children's values; a missing child of an existing node takes the reference's rule with the PARENT's
 * g:  leaf if  1 - g > g hn_g^((k^(D-depth) - 1)/(k - 1) - 1)  (depth = the parent's), otherwise the root of a full
 * subtree.  Below a missing node, map_leaf is 1 at depth D and 0 above it (the full subtree).  The root must exist. */
int ctree_map(int k, int D, const void* g_dev, const void* exists_dev, double hn_g, void* map_leaf_dev, void* work_dev,
              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTREE_H */
