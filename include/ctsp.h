/*
 * ctsp.h — C ABI of the SPARSE context-tree engine on the MI355X (gfx950), in libgmmvb.so beside ctree.h.
 *
 * ctree.h keeps the posterior in dense per-level tables and stops at k^(D+1) <= 2^24.  The engine below computes the same
 * batch update ("Context tree") on tables that hold only the nodes that exist: one open-addressing hash table
 * per level.  The node arithmetic is ctree_kernels.h's, called from here.
 *
 * Conventions are ctree.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t passed
 * as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the return
 * value is a status code (same values as enum gmmvb_status) and ctsp_last_error() gives a thread-local message.  Arguments
 * are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * Keys.  With b = max(1, ceil(log2 k)) bits per symbol the context (x[i-1], ..., x[i-D]) is one 64-bit word of b D bits,
 * the nearest symbol most significant:  key_D = sum_{j=1..D} x[i-j] << b (D - j).  The key of the same context at level d
 * is key_D with everything below its top b d bits cleared; the parent of a level-d key clears b more bits, child c of a
 * level-d key sets  c << b (D - d - 1).  The root's key is 0.  Keys of one level compare like their contexts read from the
 * nearest symbol on, which is the canonical order of every read-out.
 *
 * Limit: k <= CTSP_MAX_K and b D <= CTSP_MAX_KEY_BITS = 63.  Bit 63 is never set in a key, so the all-ones word marks an
 * empty slot and a signed 64-bit sort orders keys.  (Using the 64th bit would need a second empty mark, a valid-flag array
 * claimed by its own compare-and-swap and read before the key; nobody has asked for b D = 64 yet.)  Beyond the limit every
 * entry point returns CTSP_EUNSUPPORTED.
 *
 * Tables.  Level d = 0..D has a table of cap[d] slots, cap[d] a power of two >= 2; the levels lie back to back in every
 * array, level d starting at slot off[d] (`off`: D + 2 int64 on the HOST, off[0] = 0, off[d + 1] = off[d] + cap[d]).
 *   key[slots] uint64 (CTSP_EMPTY_KEY = no key), beta[slots][k] and g[slots] binary64, exists[slots] and leaf[slots] uint8;
 *   per-update scratch: cnt[slots][k] int64 and lnw[slots] binary64.
 * A slot whose key is set but whose exists is 0 is NOT a node: the count claims slots before the host knows whether the
 * sample is accepted, and a refused sample leaves only such slots behind.
 *
 * No floating-point atomics, no device-side recursion, no grid-wide waits, no loop that waits on another thread.  A
 * find-or-insert is a probe sequence of at most cap[d] steps; each step finds the key, claims an empty slot with a 64-bit
 * compare-and-swap, or moves on; exhaustion sets status[2].  Every slot index is masked to its table, and a symbol outside
 * 0..k-1 is never packed into a key or used as an index.
 *
 * status_dev: 4 int64 on the device, [ n | bad | overflow | 0 ].  ctsp_count zeroes it; the others only raise overflow.
 */
#ifndef CTSP_H
#define CTSP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTSP_ABI_VERSION 1
#define CTSP_MAX_K 256
#define CTSP_MAX_KEY_BITS 63
#define CTSP_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull
#define CTSP_STATUS_LEN 4

enum ctsp_status { CTSP_OK = 0, CTSP_EINVAL = 1, CTSP_EUNSUPPORTED = 2, CTSP_EHIP = 3 };
enum ctsp_dtype { CTSP_U8 = 0, CTSP_I32 = 1, CTSP_I64 = 2 };

int ctsp_abi_version(void);
const char* ctsp_last_error(void);

/* b = max(1, ceil(log2 k)); -1 for k < 1 or k > CTSP_MAX_K. */
int ctsp_symbol_bits(int k);
/* b D, the width of a key; -1 for k < 1, D < 1 or a (k, D) beyond the limit. */
int ctsp_key_bits(int k, int D);
/* The capacity that level `level` needs so that `present` claimed slots plus the at most min(n, k^level) new ones of an
 * update of n samples load it to at most 1/2: the smallest power of two >= max(2 need, floor_cap, 2), need capped at
 * k^level.  -1 for bad arguments (present < 0, n < 0, floor_cap < 0, level outside 0..D, (k, D) as above). */
int64_t ctsp_capacity(int k, int D, int level, int64_t present, int64_t n, int64_t floor_cap);
/* Bytes per slot over all seven arrays: 8 + 8 k + 8 + 1 + 1 + 8 k + 8; -1 for k outside 1..CTSP_MAX_K. */
int64_t ctsp_slot_bytes(int k);

/* Zeroes status, cnt and lnw of every slot, then counts the deepest level: one lane per sample i >= D packs the key of
 * (x[i-1], ..., x[i-D]), finds or inserts it in level D and adds 1 to cnt[slot][x[i]]; equal (key, symbol) pairs of a wave
 * are added once with their multiplicity.  status = [ n | bad | overflow | 0 ]; a sample with a bad value anywhere in
 * x[i-D..i] is dropped.  x_dev: n >= 1 symbols of `dtype`, aligned to the element size. */
int ctsp_count(int dtype, const void* x_dev, int64_t n, int k, int D, const int64_t* off, void* key_dev, void* cnt_dev,
               void* lnw_dev, void* status_dev, void* stream);

/* Levels D-1, ..., 0, one launch each: every non-zero cnt of level d + 1 is added to its parent's row (found or inserted),
 * then the head sample of level d (x[d] in the context x[d-1], ..., x[0]; head_dev: the first n_head = min(n, D) symbols as
 * int32, may be NULL when n_head = 0) adds its one count to its own node. */
int ctsp_levelup(int k, int D, const int64_t* off, void* key_dev, void* cnt_dev, const void* head_dev, int n_head,
                 void* status_dev, void* stream);

/* The up-sweep on the counts, levels D, ..., 0, one launch each, one lane per slot.  A slot whose count row sums to zero is
 * left bit-identical; every other one gets beta += cnt, its new g, exists = 1 (and leaf = 1 when created at depth D).  A
 * slot with exists = 0 reads hn_beta_dev[k] (device) and hn_g (0 at depth D).  S is summed over the children c = 0..k-1 in
 * that order, each found by lookup; an absent child adds nothing. */
int ctsp_sweep(int k, int D, const int64_t* off, const void* key_dev, const void* cnt_dev, void* lnw_dev, void* beta_dev,
               void* g_dev, void* exists_dev, void* leaf_dev, const void* head_dev, int n_head, double hn_g,
               const void* hn_beta_dev, void* stream);

/* The MAP sweep of ctree_map with children found by lookup: map_leaf_dev[slot] (uint8) of every existing node; other slots
 * are left as they are.  val_dev: binary64 scratch, one per slot (lnw may serve). */
int ctsp_map(int k, int D, const int64_t* off, const void* key_dev, const void* g_dev, const void* exists_dev, double hn_g,
             void* val_dev, void* map_leaf_dev, void* stream);

/* slot_dev[q] (int64, an index into the back-to-back arrays) of the key q_key_dev[q] (uint64) at level q_level_dev[q]
 * (int32), nq >= 1 queries; -1 for an absent key, a level outside 0..D or a key with bits set outside its level's.  With
 * insert != 0 an absent key claims a slot (exists stays as it is: the caller writes the row). */
int ctsp_find(int k, int D, const int64_t* off, void* key_dev, int64_t nq, const void* q_level_dev, const void* q_key_dev,
              int insert, void* slot_dev, void* status_dev, void* stream);

/* Growth: every NODE (key set and exists != 0) of the old tables moves to the new ones, level by level; slots that are not
 * nodes are dropped.  The new tables must be cleared by the caller (key = CTSP_EMPTY_KEY, exists = leaf = 0). */
int ctsp_rehash(int k, int D, const int64_t* off_old, const void* key_old_dev, const void* beta_old_dev,
                const void* g_old_dev, const void* exists_old_dev, const void* leaf_old_dev, const int64_t* off_new,
                void* key_new_dev, void* beta_new_dev, void* g_new_dev, void* exists_new_dev, void* leaf_new_dev,
                void* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTSP_H */
