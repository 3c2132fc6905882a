// include/regvb.h: regvb_stats, regvb_stats_window (kernels (a) and (b) of regvb_kernels.h) and the family's bookkeeping.
#include "regvb_internal.h"

#include <type_traits>

namespace regvb {
ENTRY_SAME_CODES(REGVB);
thread_local entry::Err g_err = {""};

template <typename SRC>
static int launch_gram(const SRC& src, int D, int64_t n_rows, double* stats, double* work, hipStream_t st) {
    const int T = even_tiles(D);
    // row ranges: whole batches, at most gram_max_splits(T) of them, the same for the same n_rows (run-to-run identical sums)
    const int max_splits = gram_max_splits(T);
    int64_t rps = (n_rows + max_splits - 1) / max_splits;
    rps = (rps + kBatch - 1) / kBatch * kBatch;
    const int S = (int)((n_rows + rps - 1) / rps);
    for_tiles(T, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        hipLaunchKernelGGL((gram_kernel<TT, SRC>), dim3(S), dim3(32 * TT), 0, st, src, n_rows, rps, work);
    });
    if (int rc = g_err.launched("gram_kernel launch")) return rc;
    const int64_t len = (int64_t)D * D + D + 2;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(entry::grid_of(len, 256)), dim3(256), 0, st, work, S, T, D, stats);
    return g_err.launched("gram_reduce_kernel launch");
}
}  // namespace regvb

using namespace regvb;

extern "C" {

int regvb_abi_version(void) { return REGVB_ABI_VERSION; }
const char* regvb_last_error(void) { return g_err.msg; }

int64_t regvb_stats_len(int D) {
    if (D < 1 || D > REGVB_MAX_DEGREE) return -1;
    return (int64_t)D * D + D + 2;
}

int64_t regvb_stats_work_len(int D) {
    if (D < 1 || D > REGVB_MAX_DEGREE) return -1;
    return gram_max_splits(even_tiles(D)) * gram_slab_len(even_tiles(D));
}

int regvb_stats(int D, int x_dtype, const void* x_dev, int64_t ldx, int y_dtype, const void* y_dev, int64_t n_rows,
                double* stats_dev, double* work_dev, void* stream) {
    if (D < 1) return g_err.fail(REGVB_EINVAL, "regvb_stats: D must be >= 1");
    if (D > REGVB_MAX_DEGREE) return g_err.fail(REGVB_EUNSUPPORTED, "regvb_stats: D > 256 is not supported");
    if (x_dtype != REGVB_F32 && x_dtype != REGVB_F64)
        return g_err.fail(REGVB_EINVAL, "regvb_stats: x_dtype must be REGVB_F32 or REGVB_F64");
    if (y_dtype != REGVB_F32 && y_dtype != REGVB_F64)
        return g_err.fail(REGVB_EINVAL, "regvb_stats: y_dtype must be REGVB_F32 or REGVB_F64");
    if (n_rows < 1) return g_err.fail(REGVB_EINVAL, "regvb_stats: n_rows must be >= 1");
    if (ldx < D) return g_err.fail(REGVB_EINVAL, "regvb_stats: ldx must be >= D");
    if (!x_dev || !y_dev || !stats_dev || !work_dev) return g_err.fail(REGVB_EINVAL, "regvb_stats: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const float* xf = (const float*)x_dev;
    const double* xd = (const double*)x_dev;
    const float* yf = (const float*)y_dev;
    const double* yd = (const double*)y_dev;
    if (x_dtype == REGVB_F32 && y_dtype == REGVB_F32)
        return launch_gram(MatrixRows<float, float>{xf, ldx, yf, D}, D, n_rows, stats_dev, work_dev, st);
    if (x_dtype == REGVB_F32) return launch_gram(MatrixRows<float, double>{xf, ldx, yd, D}, D, n_rows, stats_dev, work_dev, st);
    if (y_dtype == REGVB_F32) return launch_gram(MatrixRows<double, float>{xd, ldx, yf, D}, D, n_rows, stats_dev, work_dev, st);
    return launch_gram(MatrixRows<double, double>{xd, ldx, yd, D}, D, n_rows, stats_dev, work_dev, st);
}

int regvb_stats_window(int p, int x_dtype, const void* series_dev, int64_t length, int padding,
                       double* stats_dev, double* work_dev, void* stream) {
    if (p < 0) return g_err.fail(REGVB_EINVAL, "regvb_stats_window: p must be >= 0");
    if (p + 1 > REGVB_MAX_DEGREE) return g_err.fail(REGVB_EUNSUPPORTED, "regvb_stats_window: p + 1 > 256 is not supported");
    if (x_dtype != REGVB_F32 && x_dtype != REGVB_F64)
        return g_err.fail(REGVB_EINVAL, "regvb_stats_window: x_dtype must be REGVB_F32 or REGVB_F64");
    if (padding != REGVB_PAD_NONE && padding != REGVB_PAD_ZEROS)
        return g_err.fail(REGVB_EINVAL, "regvb_stats_window: padding must be REGVB_PAD_NONE or REGVB_PAD_ZEROS");
    if (length <= p) return g_err.fail(REGVB_EINVAL, "regvb_stats_window: length must be > p");
    if (!series_dev || !stats_dev || !work_dev) return g_err.fail(REGVB_EINVAL, "regvb_stats_window: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t t0 = padding == REGVB_PAD_ZEROS ? 0 : p;
    const int64_t n_rows = length - t0;
    if (x_dtype == REGVB_F32)
        return launch_gram(WindowRows<float>{(const float*)series_dev, p, t0}, p + 1, n_rows, stats_dev, work_dev, st);
    return launch_gram(WindowRows<double>{(const double*)series_dev, p, t0}, p + 1, n_rows, stats_dev, work_dev, st);
}

}  // extern "C"
