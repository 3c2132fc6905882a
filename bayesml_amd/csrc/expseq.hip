// include/expseq.h: argument checks and the three launches (aggregate, scan, emit) of expseq_kernels.h.
#include "../../include/expseq.h"
#include "../../include/expfam.h"
#include "entry.h"
#include "expseq_kernels.h"

namespace expseq {
using namespace entry;
ENTRY_SAME_CODES(EXPSEQ);
static_assert(EXPSEQ_TILE == kTile && EXPSEQ_SCAN_THREADS == kScanThreads && kScanThreads == kThreads, "expseq.h constants");
static thread_local Err g_err = {""};

static bool is_int_dtype(int d) { return d == EXPFAM_U8 || d == EXPFAM_I32 || d == EXPFAM_I64; }
static bool is_float_dtype(int d) { return d == EXPFAM_F32 || d == EXPFAM_F64; }
static int elem_size(int d) { return d == EXPFAM_U8 ? 1 : (d == EXPFAM_I32 || d == EXPFAM_F32) ? 4 : 8; }
static int64_t tiles_of(int64_t m) { return (m + kTile - 1) / kTile; }

// The checks every entry point shares; `ints` says which dtypes the family reads, the first `pos0` start slots may be any
// finite number and the other `npos` must be positive.
static int check_common(const char* who, bool ints, int dtype, const void* x, int64_t n, const double* start, int pos0, int npos,
                        const void* status, const void* work, std::initializer_list<const double*> outs) {
    if (dtype < EXPFAM_U8 || dtype > EXPFAM_F64) return g_err.fail(EXPSEQ_EINVAL, "%s: dtype must be an expfam_dtype", who);
    if (ints ? !is_int_dtype(dtype) : !is_float_dtype(dtype))
        return g_err.fail(EXPSEQ_EINVAL, "%s: dtype must be %s", who,
                          ints ? "EXPFAM_U8, EXPFAM_I32 or EXPFAM_I64" : "EXPFAM_F32 or EXPFAM_F64");
    if (n < 1) return g_err.fail(EXPSEQ_EINVAL, "%s: n must be >= 1", who);
    if (!x || !start || !status || !work) return g_err.fail(EXPSEQ_EINVAL, "%s: null pointer", who);
    if (misaligned(x, elem_size(dtype))) return g_err.fail(EXPSEQ_EINVAL, "%s: x_dev must be aligned to its element size", who);
    if (misaligned(status, 8) || misaligned(work, 8))
        return g_err.fail(EXPSEQ_EINVAL, "%s: status_dev and work_dev must be aligned to 8 bytes", who);
    for (const double* o : outs)
        if (misaligned(o, 8)) return g_err.fail(EXPSEQ_EINVAL, "%s: an output array is not aligned to 8 bytes", who);
    for (int k = 0; k < pos0 + npos; ++k) {
        const double v = start[k];
        if (!(v - v == 0.0) || (k >= pos0 && !(v > 0.0)))
            return g_err.fail(EXPSEQ_EINVAL, "%s: start[%d] must be %s", who, k, k >= pos0 ? "positive and finite" : "finite");
    }
    return EXPSEQ_OK;
}

template <typename T, typename F>
static int launch(const void* x_dev, int64_t n, const double* start, int nstart, const Out& out, double* nats,
                  int64_t* status_dev, void* work_dev, hipStream_t st) {
    using S = typename F::S;
    const int64_t tiles = tiles_of(n);
    if (tiles > INT32_MAX) return g_err.fail(EXPSEQ_EUNSUPPORTED, "expseq: n > %lld is not supported", (long long)INT32_MAX * kTile);
    int64_t* agg = (int64_t*)work_dev;
    int64_t* carry = agg + tiles * kSlots;
    Start s = {};
    for (int k = 0; k < nstart; ++k) s.v[k] = start[k];
    const T* x = (const T*)x_dev;
    hipLaunchKernelGGL((aggregate_kernel<T, F>), dim3((unsigned)tiles), dim3(kThreads), 0, st, x, n, agg);
    if (int rc = g_err.launched("aggregate_kernel launch")) return rc;
    hipLaunchKernelGGL((scan_kernel<S>), dim3(1), dim3(kScanThreads), 0, st, (const int64_t*)agg, tiles, carry, status_dev);
    if (int rc = g_err.launched("scan_kernel launch")) return rc;
    bool any = nats != nullptr;
    for (int o = 0; o < kMaxOut; ++o) any = any || out.p[o] != nullptr;
    if (!any) return EXPSEQ_OK;          // the status alone
    hipLaunchKernelGGL((emit_kernel<T, F>), dim3((unsigned)tiles), dim3(kThreads), 0, st, x, n, (const int64_t*)carry, s, out, nats);
    return g_err.launched("emit_kernel launch");
}

template <template <typename> class F>
static int launch_ints(int dtype, const void* x, int64_t n, const double* start, int nstart, const Out& out, double* nats,
                       int64_t* status, void* work, hipStream_t st) {
    if (dtype == EXPFAM_U8) return launch<uint8_t, F<uint8_t>>(x, n, start, nstart, out, nats, status, work, st);
    if (dtype == EXPFAM_I32) return launch<int32_t, F<int32_t>>(x, n, start, nstart, out, nats, status, work, st);
    return launch<int64_t, F<int64_t>>(x, n, start, nstart, out, nats, status, work, st);
}
template <template <typename> class F>
static int launch_floats(int dtype, const void* x, int64_t n, const double* start, int nstart, const Out& out, double* nats,
                         int64_t* status, void* work, hipStream_t st) {
    if (dtype == EXPFAM_F32) return launch<float, F<float>>(x, n, start, nstart, out, nats, status, work, st);
    return launch<double, F<double>>(x, n, start, nstart, out, nats, status, work, st);
}

template <typename T>
static int launch_categorical(const T* x, int64_t m, int degree, const double* alpha, double s0, int64_t i0, int64_t* counts,
                              double* nats, double* rows, int64_t* argmax, int64_t* status, int64_t* hist, int64_t* bad,
                              hipStream_t st) {
    const int64_t tiles = tiles_of(m);
    hipLaunchKernelGGL((cat_hist_kernel<T>), dim3((unsigned)tiles), dim3(kThreads), sizeof(unsigned) * (size_t)(degree + 1), st, x, m,
                       degree, hist, bad);
    if (int rc = g_err.launched("cat_hist_kernel launch")) return rc;
    hipLaunchKernelGGL(cat_scan_kernel, dim3((unsigned)degree + 1), dim3(kThreads), 0, st, hist, (const int64_t*)bad, tiles,
                       degree, counts, status, (int)(i0 == 0));
    if (int rc = g_err.launched("cat_scan_kernel launch")) return rc;
    if (nats) {
        hipLaunchKernelGGL((cat_emit_kernel<T>), dim3((unsigned)tiles), dim3(kThreads), sizeof(long long) * (size_t)degree, st, x, m,
                           degree, (const int64_t*)hist, alpha, s0, i0, nats);
        if (int rc = g_err.launched("cat_emit_kernel launch")) return rc;
    }
    if (rows || argmax) {
        hipLaunchKernelGGL((cat_rows_kernel<T>), dim3((unsigned)tiles), dim3(64), 2 * sizeof(double) * (size_t)degree, st, x, m, degree,
                           (const int64_t*)hist, alpha, s0, i0, rows, argmax);
        if (int rc = g_err.launched("cat_rows_kernel launch")) return rc;
    }
    return EXPSEQ_OK;
}

template <typename T>
static int run_categorical(const void* x_dev, int64_t m, int degree, int onehot, int64_t ld, const double* alpha, double s0,
                           int64_t i0, int64_t* counts, double* nats, double* rows, int64_t* argmax, int64_t* status,
                           void* work_dev, hipStream_t st) {
    const int64_t tiles = tiles_of(m);
    int64_t* hist = (int64_t*)work_dev;
    int64_t* bad = hist + tiles * degree;
    if (!onehot) return launch_categorical<T>((const T*)x_dev, m, degree, alpha, s0, i0, counts, nats, rows, argmax, status, hist, bad, st);
    int64_t* idx = bad + tiles;
    hipLaunchKernelGGL((onehot_index_kernel<T>), dim3(grid_of(m, kWaves)), dim3(kThreads), 0, st, (const T*)x_dev, m, degree, ld, idx);
    if (int rc = g_err.launched("onehot_index_kernel launch")) return rc;
    return launch_categorical<int64_t>(idx, m, degree, alpha, s0, i0, counts, nats, rows, argmax, status, hist, bad, st);
}
}  // namespace expseq

using namespace expseq;

extern "C" {

int expseq_abi_version(void) { return EXPSEQ_ABI_VERSION; }
const char* expseq_last_error(void) { return g_err.msg; }

int64_t expseq_work_len(int family, int degree, int64_t m) {
    if (family < EXPSEQ_BERNOULLI || family > EXPSEQ_CATEGORICAL || m < 1) return -1;
    if (family == EXPSEQ_CATEGORICAL) {
        if (degree < 1 || degree > EXPFAM_MAX_DEGREE) return -1;
        return tiles_of(m) * ((int64_t)degree + 1) + m;
    }
    return degree != 0 ? -1 : 2 * kSlots * tiles_of(m);
}

int expseq_bernoulli(int dtype, const void* x_dev, int64_t n, const double* start, double* p_theta_dev, double* nats_dev,
                     int64_t* status_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expseq_bernoulli", true, dtype, x_dev, n, start, 0, 2, status_dev, work_dev, {p_theta_dev, nats_dev}))
        return rc;
    return launch_ints<Bernoulli>(dtype, x_dev, n, start, 2, Out{{p_theta_dev}}, nats_dev, status_dev, work_dev, (hipStream_t)stream);
}

int expseq_poisson(int dtype, const void* x_dev, int64_t n, const double* start, double* p_r_dev, double* p_theta_dev,
                   double* nats_dev, int64_t* status_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expseq_poisson", true, dtype, x_dev, n, start, 0, 2, status_dev, work_dev,
                              {p_r_dev, p_theta_dev, nats_dev}))
        return rc;
    return launch_ints<Poisson>(dtype, x_dev, n, start, 2, Out{{p_r_dev, p_theta_dev}}, nats_dev, status_dev, work_dev,
                                (hipStream_t)stream);
}

int expseq_exponential(int dtype, const void* x_dev, int64_t n, const double* start, double* p_kappa_dev,
                       double* p_lambda_dev, double* nats_dev, int64_t* status_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expseq_exponential", false, dtype, x_dev, n, start, 0, 2, status_dev, work_dev,
                              {p_kappa_dev, p_lambda_dev, nats_dev}))
        return rc;
    return launch_floats<Exponential>(dtype, x_dev, n, start, 2, Out{{p_kappa_dev, p_lambda_dev}}, nats_dev, status_dev, work_dev,
                                      (hipStream_t)stream);
}

int expseq_normal(int dtype, const void* x_dev, int64_t n, const double* start, double* p_mu_dev, double* p_nu_dev,
                  double* p_lambda_dev, double* nats_dev, int64_t* status_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expseq_normal", false, dtype, x_dev, n, start, 1, 3, status_dev, work_dev,
                              {p_mu_dev, p_nu_dev, p_lambda_dev, nats_dev}))
        return rc;
    return launch_floats<Normal>(dtype, x_dev, n, start, 4, Out{{p_mu_dev, p_nu_dev, p_lambda_dev}}, nats_dev, status_dev,
                                 work_dev, (hipStream_t)stream);
}

int expseq_categorical(int dtype, const void* x_dev, int64_t m, int degree, int onehot, int64_t ld, const double* alpha_dev,
                       double s0, int64_t i0, int64_t* counts_dev, double* nats_dev, double* rows_dev, int64_t* argmax_dev,
                       int64_t* status_dev, void* work_dev, void* stream) {
    const char* who = "expseq_categorical";
    if (degree < 1) return g_err.fail(EXPSEQ_EINVAL, "%s: degree must be >= 1", who);
    if (degree > EXPFAM_MAX_DEGREE) return g_err.fail(EXPSEQ_EUNSUPPORTED, "%s: degree > %d is not supported", who, EXPFAM_MAX_DEGREE);
    if (!is_int_dtype(dtype)) return g_err.fail(EXPSEQ_EINVAL, "%s: dtype must be EXPFAM_U8, EXPFAM_I32 or EXPFAM_I64", who);
    if (m < 1) return g_err.fail(EXPSEQ_EINVAL, "%s: m must be >= 1", who);
    if (tiles_of(m) > INT32_MAX) return g_err.fail(EXPSEQ_EUNSUPPORTED, "%s: m is too large for one call", who);
    if (i0 < 0) return g_err.fail(EXPSEQ_EINVAL, "%s: i0 must be >= 0", who);
    if (!x_dev || !alpha_dev || !counts_dev || !status_dev || !work_dev) return g_err.fail(EXPSEQ_EINVAL, "%s: null pointer", who);
    if (onehot && ld < degree) return g_err.fail(EXPSEQ_EINVAL, "%s: ld must be >= degree", who);
    if (misaligned(x_dev, elem_size(dtype))) return g_err.fail(EXPSEQ_EINVAL, "%s: x_dev must be aligned to its element size", who);
    if (any_misaligned(8, (const void*)alpha_dev, (const void*)counts_dev, (const void*)nats_dev, (const void*)rows_dev,
                       (const void*)argmax_dev, (const void*)status_dev, (const void*)work_dev))
        return g_err.fail(EXPSEQ_EINVAL, "%s: a device array is not aligned to 8 bytes", who);
    if (!(s0 - s0 == 0.0) || !(s0 > 0.0)) return g_err.fail(EXPSEQ_EINVAL, "%s: s0 must be positive and finite", who);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EXPFAM_U8)
        return run_categorical<uint8_t>(x_dev, m, degree, onehot, ld, alpha_dev, s0, i0, counts_dev, nats_dev, rows_dev, argmax_dev,
                                        status_dev, work_dev, st);
    if (dtype == EXPFAM_I32)
        return run_categorical<int32_t>(x_dev, m, degree, onehot, ld, alpha_dev, s0, i0, counts_dev, nats_dev, rows_dev, argmax_dev,
                                        status_dev, work_dev, st);
    return run_categorical<int64_t>(x_dev, m, degree, onehot, ld, alpha_dev, s0, i0, counts_dev, nats_dev, rows_dev, argmax_dev,
                                    status_dev, work_dev, st);
}

}  // extern "C"
