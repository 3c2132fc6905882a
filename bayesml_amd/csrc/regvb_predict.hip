// include/regvb.h: regvb_predict (kernel (c) of regvb_kernels.h).
#include "regvb_internal.h"

#include <type_traits>

using namespace regvb;

template <typename XT>
static int launch_predict(int D, const XT* x, int64_t ldx, int64_t n_rows, const double* mu, const double* linv, double scale,
                          double* p_ms, double* p_lambdas, double* work, hipStream_t st) {
    const int T = even_tiles(D);
    const int64_t plen = packed_len(T);
    hipLaunchKernelGGL(pack_factor_kernel, dim3(entry::grid_of(plen, 256)), dim3(256), 0, st, linv, D, T, work);
    if (int rc = g_err.launched("pack_factor_kernel launch")) return rc;
    for_tiles(T, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        constexpr int rows = 16 * predict_waves(TT);
        hipLaunchKernelGGL((predict_kernel<TT, XT>), dim3(entry::grid_of(n_rows, rows)), dim3(4 * rows), 0, st, x, ldx, n_rows, D,
                           mu, (const double*)work, scale, p_ms, p_lambdas);
    });
    return g_err.launched("predict_kernel launch");
}

extern "C" {

int64_t regvb_predict_work_len(int D) {
    if (D < 1 || D > REGVB_MAX_DEGREE) return -1;
    return packed_len(even_tiles(D));
}

int regvb_predict(int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* mu_dev,
                  const double* linv_dev, double scale, double* p_ms_dev, double* p_lambdas_dev, double* work_dev,
                  void* stream) {
    if (D < 1) return g_err.fail(REGVB_EINVAL, "regvb_predict: D must be >= 1");
    if (D > REGVB_MAX_DEGREE) return g_err.fail(REGVB_EUNSUPPORTED, "regvb_predict: D > 256 is not supported");
    if (x_dtype != REGVB_F32 && x_dtype != REGVB_F64)
        return g_err.fail(REGVB_EINVAL, "regvb_predict: x_dtype must be REGVB_F32 or REGVB_F64");
    if (n_rows < 1) return g_err.fail(REGVB_EINVAL, "regvb_predict: n_rows must be >= 1");
    if (n_rows > 64 * 2147483647LL) return g_err.fail(REGVB_EINVAL, "regvb_predict: n_rows too large for one launch");
    if (ldx < D) return g_err.fail(REGVB_EINVAL, "regvb_predict: ldx must be >= D");
    if (!(scale > 0.0)) return g_err.fail(REGVB_EINVAL, "regvb_predict: scale must be positive");
    if (!x_dev || !mu_dev || !linv_dev || !p_ms_dev || !p_lambdas_dev || !work_dev)
        return g_err.fail(REGVB_EINVAL, "regvb_predict: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == REGVB_F32)
        return launch_predict(D, (const float*)x_dev, ldx, n_rows, mu_dev, linv_dev, scale, p_ms_dev, p_lambdas_dev, work_dev, st);
    return launch_predict(D, (const double*)x_dev, ldx, n_rows, mu_dev, linv_dev, scale, p_ms_dev, p_lambdas_dev, work_dev, st);
}

}  // extern "C"
