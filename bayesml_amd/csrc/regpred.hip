// include/regpred.h: the argument checks and the launches (regpred_kernels.h).
#include "../../include/regpred.h"
#include "regvb_internal.h"
#include "regpred_kernels.h"

namespace regpred {
ENTRY_SAME_CODES(REGPRED);
static_assert(REGPRED_MAX_DEGREE == REGVB_MAX_DEGREE, "regpred.h and the kernels disagree");
static_assert((int)REGPRED_F32 == (int)REGVB_F32 && (int)REGPRED_F64 == (int)REGVB_F64 &&
                  (int)REGPRED_PAD_ZEROS == (int)REGVB_PAD_ZEROS, "regpred.h repeats regvb.h's codes");
static thread_local entry::Err g_err = {""};

struct ScoreArgs {
    int D;
    int64_t n_rows;
    const double *mu, *linv;
    StudentT k;
    double *lnp, *work;
    hipStream_t st;
};

// everything about a scoring call that does not depend on the row source
static int check_score(const char* who, const ScoreArgs& a) {
    if (a.n_rows < 1) return g_err.fail(REGPRED_EINVAL, "%s: n_rows must be >= 1", who);
    if (a.n_rows > 64 * 2147483647LL) return g_err.fail(REGPRED_EINVAL, "%s: n_rows too large for one launch", who);
    if (!(a.k.scale > 0.0)) return g_err.fail(REGPRED_EINVAL, "%s: scale must be positive", who);
    if (!(a.k.nu > 0.0)) return g_err.fail(REGPRED_EINVAL, "%s: nu must be positive", who);
    if (!(a.k.c0 == a.k.c0)) return g_err.fail(REGPRED_EINVAL, "%s: c0 must be a number", who);
    if (!a.mu || !a.linv || !a.lnp || !a.work) return g_err.fail(REGPRED_EINVAL, "%s: null pointer", who);
    if (entry::any_misaligned(8, a.mu, a.linv, a.lnp, a.work))
        return g_err.fail(REGPRED_EINVAL, "%s: the double arrays must be 8-byte aligned", who);
    return REGPRED_OK;
}

// what the two window entry points share
static int check_window(const char* who, int p, int x_dtype, const void* series, int64_t length, int padding, int64_t n_seq,
                        const int64_t* off, const int64_t* roff, int64_t n_rows) {
    if (p < 0) return g_err.fail(REGPRED_EINVAL, "%s: p must be >= 0", who);
    if (p + 1 > REGPRED_MAX_DEGREE) return g_err.fail(REGPRED_EUNSUPPORTED, "%s: p + 1 > 256 is not supported", who);
    if (x_dtype != REGPRED_F32 && x_dtype != REGPRED_F64)
        return g_err.fail(REGPRED_EINVAL, "%s: x_dtype must be REGPRED_F32 or REGPRED_F64", who);
    if (padding != REGPRED_PAD_NONE && padding != REGPRED_PAD_ZEROS)
        return g_err.fail(REGPRED_EINVAL, "%s: padding must be REGPRED_PAD_NONE or REGPRED_PAD_ZEROS", who);
    if (n_seq < 1) return g_err.fail(REGPRED_EINVAL, "%s: n_seq must be >= 1", who);
    if (n_rows < 1 || n_rows > length)
        return g_err.fail(REGPRED_EINVAL, "%s: n_rows must be in 1 .. length (every row is a value of the array)", who);
    if (!series || !off || !roff) return g_err.fail(REGPRED_EINVAL, "%s: null pointer", who);
    if (entry::misaligned(series, x_dtype == REGPRED_F32 ? 4 : 8) || entry::any_misaligned(8, off, roff))
        return g_err.fail(REGPRED_EINVAL, "%s: the series and the offset tables must be aligned to their element size", who);
    return REGPRED_OK;
}

template <typename ARG>
static int launch_score(const ARG& arg, const ScoreArgs& a) {
    const int T = regvb::even_tiles(a.D);
    hipLaunchKernelGGL(regvb::pack_factor_kernel, dim3(entry::grid_of(regvb::packed_len(T), 256)), dim3(256), 0, a.st, a.linv,
                       a.D, T, a.work);
    if (int rc = g_err.launched("pack_factor_kernel launch")) return rc;
    regvb::for_tiles(T, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        constexpr int rows = 16 * predict_waves(TT);
        hipLaunchKernelGGL((score_kernel<TT, ARG>), dim3(entry::grid_of(a.n_rows, rows)), dim3(4 * rows), 0, a.st, arg, a.n_rows,
                           a.D, a.mu, (const double*)a.work, a.k, a.lnp);
    });
    return g_err.launched("score_kernel launch");
}

// regvb_stats.hip's launch_gram over the segmented source: the same row ranges, slabs and reduce
template <typename ARG>
static int launch_seg_gram(const ARG& arg, int D, int64_t n_rows, double* stats, double* work, hipStream_t st) {
    const int T = regvb::even_tiles(D);
    const int max_splits = regvb::gram_max_splits(T);
    int64_t rps = (n_rows + max_splits - 1) / max_splits;
    rps = (rps + regvb::kBatch - 1) / regvb::kBatch * regvb::kBatch;
    const int S = (int)((n_rows + rps - 1) / rps);
    regvb::for_tiles(T, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        hipLaunchKernelGGL((seg_gram_kernel<TT, ARG>), dim3(S), dim3(32 * TT), 0, st, arg, n_rows, rps, work);
    });
    if (int rc = g_err.launched("seg_gram_kernel launch")) return rc;
    const int64_t len = (int64_t)D * D + D + 2;
    hipLaunchKernelGGL(regvb::gram_reduce_kernel, dim3(entry::grid_of(len, 256)), dim3(256), 0, st, work, S, T, D, stats);
    return g_err.launched("gram_reduce_kernel launch");
}

static int launch_sum(const int64_t* tab, int64_t chunk, int64_t n, int64_t n_seg, const double* v, double* out, hipStream_t st) {
    hipLaunchKernelGGL(segment_sum_kernel, dim3(entry::grid_of(n_seg, kSumWaves)), dim3(64 * kSumWaves), 0, st, tab, chunk, n,
                       n_seg, v, out);
    return g_err.launched("segment_sum_kernel launch");
}
}  // namespace regpred

using namespace regpred;

extern "C" {

int regpred_abi_version(void) { return REGPRED_ABI_VERSION; }
const char* regpred_last_error(void) { return g_err.msg; }

int64_t regpred_work_len(int D) {
    if (D < 1 || D > REGPRED_MAX_DEGREE) return -1;
    return regvb::packed_len(regvb::even_tiles(D));
}

int64_t regpred_stats_work_len(int D) {
    if (D < 1 || D > REGPRED_MAX_DEGREE) return -1;
    return regvb::gram_max_splits(regvb::even_tiles(D)) * regvb::gram_slab_len(regvb::even_tiles(D));
}

int64_t regpred_totals_work_len(int64_t n_rows) {
    if (n_rows < 0) return -1;
    return n_rows < REGPRED_TOTAL_CHUNK ? 1 : (n_rows + REGPRED_TOTAL_CHUNK - 1) / REGPRED_TOTAL_CHUNK;
}

int regpred_logpdf(int D, int x_dtype, const void* x_dev, int64_t ldx, int y_dtype, const void* y_dev, int64_t n_rows,
                   const double* mu_dev, const double* linv_dev, double scale, double nu, double c0, double* lnp_dev,
                   double* work_dev, void* stream) {
    const char* who = "regpred_logpdf";
    if (D < 1) return g_err.fail(REGPRED_EINVAL, "%s: D must be >= 1", who);
    if (D > REGPRED_MAX_DEGREE) return g_err.fail(REGPRED_EUNSUPPORTED, "%s: D > 256 is not supported", who);
    if (x_dtype != REGPRED_F32 && x_dtype != REGPRED_F64)
        return g_err.fail(REGPRED_EINVAL, "%s: x_dtype must be REGPRED_F32 or REGPRED_F64", who);
    if (y_dtype != REGPRED_F32 && y_dtype != REGPRED_F64)
        return g_err.fail(REGPRED_EINVAL, "%s: y_dtype must be REGPRED_F32 or REGPRED_F64", who);
    if (ldx < D) return g_err.fail(REGPRED_EINVAL, "%s: ldx must be >= D", who);
    if (!x_dev || !y_dev) return g_err.fail(REGPRED_EINVAL, "%s: null pointer", who);
    if (entry::misaligned(x_dev, x_dtype == REGPRED_F32 ? 4 : 8) || entry::misaligned(y_dev, y_dtype == REGPRED_F32 ? 4 : 8))
        return g_err.fail(REGPRED_EINVAL, "%s: x and y must be aligned to their element size", who);
    const ScoreArgs a = {D, n_rows, mu_dev, linv_dev, {scale, nu, c0}, lnp_dev, work_dev, (hipStream_t)stream};
    if (int rc = check_score(who, a)) return rc;
    const float* xf = (const float*)x_dev;
    const double* xd = (const double*)x_dev;
    const float* yf = (const float*)y_dev;
    const double* yd = (const double*)y_dev;
    if (x_dtype == REGPRED_F32 && y_dtype == REGPRED_F32) return launch_score(MatrixArgs<float, float>{{xf, ldx, yf, D}}, a);
    if (x_dtype == REGPRED_F32) return launch_score(MatrixArgs<float, double>{{xf, ldx, yd, D}}, a);
    if (y_dtype == REGPRED_F32) return launch_score(MatrixArgs<double, float>{{xd, ldx, yf, D}}, a);
    return launch_score(MatrixArgs<double, double>{{xd, ldx, yd, D}}, a);
}

int regpred_logpdf_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding, int64_t n_seq,
                          const int64_t* off_dev, const int64_t* roff_dev, int64_t n_rows, const double* mu_dev,
                          const double* linv_dev, double scale, double nu, double c0, double* lnp_dev, double* work_dev,
                          void* stream) {
    const char* who = "regpred_logpdf_window";
    if (int rc = check_window(who, p, x_dtype, series_dev, length, padding, n_seq, off_dev, roff_dev, n_rows)) return rc;
    const ScoreArgs a = {p + 1, n_rows, mu_dev, linv_dev, {scale, nu, c0}, lnp_dev, work_dev, (hipStream_t)stream};
    if (int rc = check_score(who, a)) return rc;
    const int64_t t0 = padding == REGPRED_PAD_ZEROS ? 0 : p;
    if (x_dtype == REGPRED_F32)
        return launch_score(SegWindowArgs<float>{(const float*)series_dev, length, p, t0, roff_dev, off_dev, n_seq}, a);
    return launch_score(SegWindowArgs<double>{(const double*)series_dev, length, p, t0, roff_dev, off_dev, n_seq}, a);
}

int regpred_stats_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding, int64_t n_seq,
                         const int64_t* off_dev, const int64_t* roff_dev, int64_t n_rows, double* stats_dev,
                         double* work_dev, void* stream) {
    const char* who = "regpred_stats_window";
    if (int rc = check_window(who, p, x_dtype, series_dev, length, padding, n_seq, off_dev, roff_dev, n_rows)) return rc;
    if (!stats_dev || !work_dev) return g_err.fail(REGPRED_EINVAL, "%s: null pointer", who);
    if (entry::any_misaligned(8, stats_dev, work_dev))
        return g_err.fail(REGPRED_EINVAL, "%s: the double arrays must be 8-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t t0 = padding == REGPRED_PAD_ZEROS ? 0 : p;
    if (x_dtype == REGPRED_F32)
        return launch_seg_gram(SegWindowArgs<float>{(const float*)series_dev, length, p, t0, roff_dev, off_dev, n_seq}, p + 1,
                               n_rows, stats_dev, work_dev, st);
    return launch_seg_gram(SegWindowArgs<double>{(const double*)series_dev, length, p, t0, roff_dev, off_dev, n_seq}, p + 1,
                           n_rows, stats_dev, work_dev, st);
}

int regpred_totals(int64_t n_seq, const int64_t* roff_dev, int64_t n_rows, const double* lnp_dev, double* tot_dev,
                   double* total_dev, double* work_dev, void* stream) {
    const char* who = "regpred_totals";
    if (n_rows < 0) return g_err.fail(REGPRED_EINVAL, "%s: n_rows must be >= 0", who);
    if (!tot_dev && !total_dev) return g_err.fail(REGPRED_EINVAL, "%s: neither tot_dev nor total_dev is given", who);
    if (tot_dev && n_seq < 1) return g_err.fail(REGPRED_EINVAL, "%s: n_seq must be >= 1", who);
    if (tot_dev && n_seq > kSumWaves * 2147483647LL)
        return g_err.fail(REGPRED_EINVAL, "%s: n_seq too large for one launch", who);
    if ((tot_dev && !roff_dev) || (total_dev && !work_dev) || (n_rows > 0 && !lnp_dev))
        return g_err.fail(REGPRED_EINVAL, "%s: null pointer", who);
    if (entry::any_misaligned(8, roff_dev, lnp_dev, tot_dev, total_dev, work_dev))
        return g_err.fail(REGPRED_EINVAL, "%s: the arrays must be 8-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    if (tot_dev)
        if (int rc = launch_sum(roff_dev, 0, n_rows, n_seq, lnp_dev, tot_dev, st)) return rc;
    if (!total_dev) return REGPRED_OK;
    const int64_t chunks = (n_rows + REGPRED_TOTAL_CHUNK - 1) / REGPRED_TOTAL_CHUNK;
    if (chunks > 0)
        if (int rc = launch_sum(nullptr, REGPRED_TOTAL_CHUNK, n_rows, chunks, lnp_dev, work_dev, st)) return rc;
    return launch_sum(nullptr, chunks, chunks, 1, work_dev, total_dev, st);      // (no rows: an empty segment, 0.0)
}

}  // extern "C"
