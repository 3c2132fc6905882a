/*
 * ctfit.h — C ABI of the many-sequence fit of the context tree on the MI355X (gfx950), in libgmmvb.so beside ctree.h,
 * ctsp.h, ctseq.h and ctpred.h.
 *
 * The reference (bayesml/BayesML v0.3.1, bayesml/contexttree/_contexttree.py:688-731) learns one sequence per call; a
 * batch of S independent sequences is the loop  for s in seqs: update_posterior(s)  on one model.  ctree.h's count and
 * sweep collapse time under the assumption of one "head" per level (the sample i = d whose path ends at depth d < D).
 * With S sequences there are up to S * D heads, interleaved in time with ordinary visits of the same nodes; the entry points
 * below count the visits that precede every head and carry their product through the sweep ("Fit from many
 * sequences").  Dense tables only; layouts, keys and notation are ctree.h's.
 *
 * Conventions are ctree.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the
 * return value is a status code (same values as enum ctree_status) and ctfit_last_error() gives a thread-local message.
 * Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * No floating-point atomics, no device-side recursion, no grid-wide waits: counts, head counts and ranks are 64-bit
 * integers, sums of logarithms run in a fixed order that depends on the number of their terms alone.  Every index is
 * range-checked on the device before use; a symbol outside 0..k-1 is counted into `bad` and read as symbol 0: it is never
 * used as an index, and what the calls then leave in their scratch means nothing.
 *
 * Sequences.  seq_off_dev: S + 1 ascending int64, seq_off[0] = 0 and seq_off[S] = n, the starts of the sequences (equal
 * neighbours: a sequence of length 0).  hoff_dev: S + 1 int64, the exclusive prefix of min(len_s, D): sequence s owns the
 * head slots hoff[s] .. hoff[s + 1] - 1, one per depth, and H = hoff[S] is the number of heads.
 *
 * One update is  ctfit_count -> the caller sorts the two halves of keys_dev, each ascending as unsigned 64-bit integers ->
 * ctfit_rank -> ctfit_sweep;  the tables are first written by ctfit_sweep.
 *
 * Limits: ctree.h's, and n, S < 2^31.  Beyond them CTFIT_EUNSUPPORTED.
 */
#ifndef CTFIT_H
#define CTFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTFIT_ABI_VERSION 1
/* Positions per tile of the passes over the sample. */
#define CTFIT_TILE 256
/* Entries of seq_off that a tile stages in LDS; a tile that touches more sequences bisects seq_off in global memory. */
#define CTFIT_SEQ_STAGE 512
/* A node's lead is summed by one lane up to this many heads, by a workgroup's fixed tree above it. */
#define CTFIT_SERIAL_RUN 32

enum ctfit_status { CTFIT_OK = 0, CTFIT_EINVAL = 1, CTFIT_EUNSUPPORTED = 2, CTFIT_EHIP = 3 };
enum ctfit_dtype { CTFIT_U8 = 0, CTFIT_I32 = 1, CTFIT_I64 = 2 };

int ctfit_abi_version(void);
const char* ctfit_last_error(void);

/* 8-byte slots of the scratch work_dev that the three calls of one update share; -1 for a (k, D) ctree.h refuses. */
int64_t ctfit_work_len(int k, int D);
/* 8-byte slots of the scratch head_dev of ctfit_rank for H heads; -1 for H outside 1..2^31-1. */
int64_t ctfit_head_len(int64_t H);

/* Counts of the deepest level and the head records.  x_dev: n >= 1 symbols of `dtype`, aligned to the element size.
 * out_dev: 2 + k^(D+1) int64 slots  [ n | bad | cnt_D[k^D][k] ],  cnt_D[s][a] = number of positions with e = D, context key
 * s and symbol a.  keys_dev: 2 H unsigned 64-bit slots; head slot h of node v (index in the all-levels table) with symbol a
 * gets  keys[h] = v << 40 | h << 8 | a  and  keys[H + h] = (v k + a) << 32 | h.  work_dev receives the heads' counts per
 * (node, symbol) of levels 0..D-1 and a flag per node that has heads.  H = 0 (every sequence is empty) is refused. */
int ctfit_count(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, const void* hoff_dev, int64_t S, int64_t H,
                int k, int D, void* out_dev, void* keys_dev, void* work_dev, void* stream);

/* The ranks of every head and lead of every node.  keys_sorted_dev: ctfit_count's keys, each half sorted.  Every visit
 * (position, depth <= min(e, D - 1)) of a node with heads finds the node's first head of a later sequence in both orders
 * and adds 1 to its bucket; an inclusive scan turns the buckets into r (earlier visits of the node) and r_a (those with
 * the head's symbol), and  lead = sum over the node's heads, in time order, of ln((b0[a] + r_a) / (sum b0 + r))  goes to
 * work_dev.  b0 is the node's row of beta_dev where exists_dev is set, hn_beta_dev[k] otherwise.  Nothing is written to the
 * tables. */
int ctfit_rank(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, const void* hoff_dev, int64_t S, int64_t H,
               int k, int D, const void* keys_sorted_dev, const void* beta_dev, const void* exists_dev,
               const void* hn_beta_dev, void* head_dev, void* work_dev, void* stream);

/* The up-sweep, in place, as ctree_sweep: cnt_dev is out_dev + 2 slots of ctfit_count.  Level D: lnW = lnDM(b0, cnt).
 * Level d < D: cnt = child sums + head counts;  A = ln(1 - g0) + lnDM(b0, cnt) - lead,  B = ln g0 + sum of the children's
 * lnW,  g <- exp(B - logaddexp(A, B)),  lnW = lead + logaddexp(A, B);  a node whose visits are all head visits keeps its g
 * bit for bit and has lnW = lead.  Every visited node gets beta += cnt and exists = 1; a node whose count row sums to zero
 * is left bit-identical. */
int ctfit_sweep(int k, int D, const void* cnt_dev, void* beta_dev, void* g_dev, void* exists_dev, double hn_g,
                const void* hn_beta_dev, void* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTFIT_H */
