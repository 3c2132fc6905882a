/*
 * expfam.h — C ABI of the scalar conjugate families' data pass on the MI355X (gfx950), in libgmmvb.so beside gmmvb.h
 * and regvb.h.
 *
 * The reference (bayesml/BayesML v0.3.1) validates a sample on the host and then sums over it one to three times; these
 * entry points do both in ONE streaming pass over a device array and return a few 8-byte numbers:
 *
 *   ints_of_01, count_nonzero(x == 1), (x == 0)           bayesml/bernoulli/_bernoulli.py:296-310      (expfam_stats_bernoulli)
 *   nonneg_ints, np.max, count_nonzero(x == k) per k      bayesml/categorical/_categorical.py:334-364  (expfam_stats_counts)
 *   onehot_vecs, x.sum(axis=0)                            bayesml/categorical/_categorical.py:329-360  (expfam_stats_onehot)
 *   nonneg_ints, np.sum(x), gammaln(x + 1).sum()          bayesml/poisson/_poisson.py:296-314          (expfam_stats_poisson)
 *   pos_floats, np.sum(x)                                 bayesml/exponential/_exponential.py:296-313  (expfam_stats_exponential)
 *   np.sum(x) / n, np.sum((x - x_bar)**2)                 bayesml/normal/_normal.py:376-383            (expfam_stats_normal)
 *
 * Conventions are regvb.h's: pointers named *_dev are DEVICE pointers owned by the caller, `stream` is a hipStream_t
 * passed as void* (NULL = the null stream); calls only enqueue work, never allocate, never throw, never synchronise; the
 * return value is a status code (same values as enum gmmvb_status) and expfam_last_error() gives a thread-local message.
 * Arguments are validated before anything touches the device, so bad arguments are reported without a GPU.
 *
 * The sample stays in its storage dtype.  Every result is an 8-byte slot: counts and integer sums are int64, the rest is
 * IEEE binary64; `stats_dev` and `work_dev` are arrays of such slots.  A value outside the family's domain is counted in
 * `bad`, left out of every sum and never used as an index.  No sum uses floating-point atomics: every workgroup owns a
 * contiguous range and writes one slab, a second kernel combines the slabs in range order, so two calls on the same input
 * give the same bits.  (Integer atomics are used on LDS only, for histogram bins: exact and order-free.)
 */
#ifndef EXPFAM_H
#define EXPFAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXPFAM_ABI_VERSION 1
/* Largest `degree` of the two categorical passes: 4096 int64 bins are 32 KiB of LDS per workgroup, so that at the limit
 * four workgroups (and always at least two) fit the 160 KiB of a CU. */
#define EXPFAM_MAX_DEGREE 4096

enum expfam_status { EXPFAM_OK = 0, EXPFAM_EINVAL = 1, EXPFAM_EUNSUPPORTED = 2, EXPFAM_EHIP = 3 };
enum expfam_dtype { EXPFAM_U8 = 0, EXPFAM_I32 = 1, EXPFAM_I64 = 2, EXPFAM_F32 = 3, EXPFAM_F64 = 4 };
enum expfam_family {
    EXPFAM_BERNOULLI = 0, EXPFAM_COUNTS = 1, EXPFAM_ONEHOT = 2, EXPFAM_POISSON = 3, EXPFAM_EXPONENTIAL = 4, EXPFAM_NORMAL = 5
};

int expfam_abi_version(void);
const char* expfam_last_error(void);

/* Slots of a family's statistics block (`degree` is read for EXPFAM_COUNTS and EXPFAM_ONEHOT only); -1 for an unknown
 * family or a degree outside 1..EXPFAM_MAX_DEGREE.  The layouts, slot by slot (i = int64, d = binary64):
 *
 *   EXPFAM_BERNOULLI    [ n i | bad i | n1 i | n0 i ]                    bad = values outside {0, 1}
 *   EXPFAM_COUNTS       [ n i | bad i | max i | counts[degree] i ]       bad = values < 0 or >= degree; max over ALL values
 *   EXPFAM_ONEHOT       [ n i | bad i | counts[degree] i ]               n = rows; bad = rows with a negative entry or a sum != 1;
 *                                                                        counts = column sums over the good rows
 *   EXPFAM_POISSON      [ n i | bad i | sum i | sum_lgamma d ]           bad = values < 0; sum_lgamma = sum lgamma(x + 1)
 *   EXPFAM_EXPONENTIAL  [ n i | bad i | sum d ]                          bad = values for which x > 0 is false (NaN, 0, -0.0)
 *   EXPFAM_NORMAL       [ n i | mean d | m2 d ]                          m2 = sum (x - mean)^2
 *
 * Blocks of two samples combine to the block of their union: counts and sums add, `max` is the larger, and the normal
 * block merges by  n = na + nb,  mean = mean_a + (mean_b - mean_a) nb / n,  m2 = m2a + m2b + (mean_b - mean_a)^2 na nb / n. */
int64_t expfam_stats_len(int family, int degree);
/* Slots of scratch a family's pass needs: one slab per workgroup, at most 1024 workgroups.  Independent of n. */
int64_t expfam_work_len(int family, int degree);

/* Integer families read EXPFAM_U8, EXPFAM_I32 or EXPFAM_I64; the float families EXPFAM_F32 or EXPFAM_F64.  x_dev must be
 * aligned to its element size; n >= 1. */
int expfam_stats_bernoulli(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream);
int expfam_stats_counts(int dtype, const void* x_dev, int64_t n, int degree, void* stats_dev, void* work_dev, void* stream);
/* Rows x[n][degree] with row stride ld >= degree elements.  A row is read as the 16-byte ALIGNED blocks of memory that hold a
 * part of it: up to 15 bytes before the first and after the last row are read (never past a page of the rows) and ignored. */
int expfam_stats_onehot(int dtype, const void* x_dev, int64_t n, int degree, int64_t ld, void* stats_dev, void* work_dev,
                        void* stream);
int expfam_stats_poisson(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream);
int expfam_stats_exponential(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream);
int expfam_stats_normal(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXPFAM_H */
