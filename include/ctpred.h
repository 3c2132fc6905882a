/*
 * ctpred.h — C ABI of the fixed-posterior predictive engine of the context tree on the MI355X (gfx950), in libgmmvb.so
 * beside ctree.h, ctsp.h and ctseq.h.
 *
 * The reference (bayesml/BayesML v0.3.1, bayesml/contexttree/_contexttree.py:954-989) gives the predictive distribution of
 * one position from the posterior as it stands: walk the path of the context to depth e, p = beta_e / sum(beta_e) at its
 * end, then p = (1 - g_d) beta_d / sum(beta_d) + g_d p for d = e - 1, ..., 0.  The entry points below do that for every
 * position of a held-out sample at once, with nothing learnt and nothing written to the tables (DESIGN.md §4h,
 * "Predictive log-probability of held-out sequences").  One engine serves the dense tables of ctree.h and the hash tables
 * of ctsp.h; layouts, keys and notation are theirs.
 *
 * Conventions are ctree.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the
 * return value is a status code (same values as enum ctree_status) and ctpred_last_error() gives a thread-local message.
 * Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * No floating-point atomics, no device-side recursion, no grid-wide waits.  Every table index is range-checked on the
 * device before use, a hash probe is bounded by its level's capacity, and a symbol outside 0..k-1 is counted into the
 * status word and read as symbol 0: it is never used as an index, and what the call then computes means nothing.
 *
 * Row sums.  rowsum_dev has one binary64 per table slot plus one: rowsum[slot] = sum_a beta[slot][a] of every slot that
 * holds a node, and rowsum[slots] the sum of hn_beta.  The summation order is a function of k alone (ctpred_group_width(k)
 * lanes, lane l adds the entries l, l + W, l + 2W, l + 3W in this order, then a butterfly over the lanes), so the dense and
 * the sparse tables of one tree give the same bits.  Slots that hold no node are left as they are and never read.
 *
 * Limits: ctree.h's for the dense entry points, ctsp.h's for the sparse ones; CTPRED_EUNSUPPORTED beyond them.
 */
#ifndef CTPRED_H
#define CTPRED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTPRED_ABI_VERSION 1
/* Lanes per workgroup of every kernel: positions per workgroup of the scalar pass. */
#define CTPRED_TILE 256
/* Positions of one sequence that one workgroup of ctpred_totals sums; longer sequences are cut in pieces of this length. */
#define CTPRED_PIECE 4096
#define CTPRED_STATUS_LEN 2

enum ctpred_status { CTPRED_OK = 0, CTPRED_EINVAL = 1, CTPRED_EUNSUPPORTED = 2, CTPRED_EHIP = 3 };
enum ctpred_dtype { CTPRED_U8 = 0, CTPRED_I32 = 1, CTPRED_I64 = 2 };
/* How the sparse pass finds a path's nodes again on the way up: from a stack of slots in LDS, filled on the way down
 * (which stops probing below the first missing node), or by one probe per level on the way up. */
enum ctpred_upwalk { CTPRED_UP_STACK = 0, CTPRED_UP_PROBE = 1 };

int ctpred_abi_version(void);
const char* ctpred_last_error(void);

/* W = min(64, 2^ceil(log2 k)): the lanes that share one row; -1 for k outside 1..256. */
int ctpred_group_width(int k);

/* Row sums of the dense tables (k^0 + ... + k^D slots) and of hn_beta_dev[k]; rowsum_dev: slots + 1 binary64.
 * has_tree = 0: only the default row's sum is written and no table is read (beta_dev and exists_dev may be NULL). */
int ctpred_rowsum_dense(int k, int D, int has_tree, const void* beta_dev, const void* exists_dev, const void* hn_beta_dev,
                        void* rowsum_dev, void* stream);
/* The same on ctsp.h's tables (`off`: D + 2 int64 on the HOST, off[D + 1] slots); a slot holds a node when its key is set
 * and its exists is not 0. */
int ctpred_rowsum_sparse(int k, int D, int has_tree, const int64_t* off, const void* key_dev, const void* beta_dev,
                         const void* exists_dev, const void* hn_beta_dev, void* rowsum_dev, void* stream);

/* Every position i of x_dev[0..n-1] (`dtype`, aligned to the element size, read where it lies) under the fixed tables.
 * seq_off_dev: S + 1 ascending int64 on the device, seq_off[0] = 0 and seq_off[S] = n, the starts of S independent
 * sequences (equal neighbours: a sequence of length 0), or NULL with S = 0 for one sequence.  The context of position i
 * reaches back to depth e(i) = min(i - start(i), D).  A node with exists = 0 reads hn_beta_dev[k] (device) and hn_g (0 at
 * depth D); the leaf flag plays no part.  has_tree = 0: every node is missing and no table is read.
 * Outputs, each may be NULL but not all three: lnp_dev[n] binary64, ln of the probability of x[i]; argmax_dev[n] int64,
 * the first maximum of position i's distribution; rows_dev[n][k] binary64, the distributions.  lnp comes from a pass of one
 * lane per position; argmax and rows from a second pass of ctpred_group_width(k) lanes per position.
 * status_dev: CTPRED_STATUS_LEN int64, zeroed by the call, then [ n | symbols outside 0..k-1 ]. */
int ctpred_pass_dense(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, int64_t S, int k, int D, int has_tree,
                      const void* beta_dev, const void* g_dev, const void* exists_dev, const void* rowsum_dev, double hn_g,
                      const void* hn_beta_dev, void* lnp_dev, void* argmax_dev, void* rows_dev, void* status_dev, void* stream);
int ctpred_pass_sparse(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, int64_t S, int k, int D, int has_tree,
                       const int64_t* off, const void* key_dev, const void* beta_dev, const void* g_dev,
                       const void* exists_dev, const void* rowsum_dev, double hn_g, const void* hn_beta_dev, int upwalk,
                       void* lnp_dev, void* argmax_dev, void* rows_dev, void* status_dev, void* stream);

/* Pieces that the S sequences of seq_off (HOST, S + 1 int64 as above) are cut into: sum_s ceil(len_s / CTPRED_PIECE);
 * piece_off (HOST, S + 1 int64, may be NULL) receives the first piece of every sequence.  -1 for bad arguments. */
int64_t ctpred_plan_pieces(const int64_t* seq_off, int64_t S, int64_t* piece_off);

/* totals_dev[s] = sum of lnp_dev over sequence s, 0.0 for an empty one, S >= 1.  Stage one: a workgroup per piece adds its
 * positions on a fixed tree into partial_dev[pieces]; stage two: a wave per sequence adds the sequence's partials on a
 * fixed tree.  Both trees depend on the sequence's length alone.  piece_off_dev: ctpred_plan_pieces' table on the device
 * (may be NULL, with partial_dev, when pieces = 0). */
int ctpred_totals(const void* lnp_dev, int64_t n, const void* seq_off_dev, const void* piece_off_dev, int64_t S,
                  int64_t pieces, void* partial_dev, void* totals_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTPRED_H */
