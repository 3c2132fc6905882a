// include/expfam.h: argument checks, the split of a sample into workgroup ranges, and the launches of expfam_kernels.h.
#include "../../include/expfam.h"
#include "entry.h"
#include "expfam_kernels.h"

namespace expfam {
using namespace entry;
ENTRY_SAME_CODES(EXPFAM);
static thread_local Err g_err = {""};

static bool is_int_dtype(int d) { return d == EXPFAM_U8 || d == EXPFAM_I32 || d == EXPFAM_I64; }
static bool is_float_dtype(int d) { return d == EXPFAM_F32 || d == EXPFAM_F64; }
static int elem_size(int d) { return d == EXPFAM_U8 ? 1 : (d == EXPFAM_I32 || d == EXPFAM_F32) ? 4 : 8; }
static bool has_degree(int family) { return family == EXPFAM_COUNTS || family == EXPFAM_ONEHOT; }

// slots of a workgroup's slab (the statistics block without its leading n; the normal family's slab is n, mean - shift, m2, shift)
static int slab_len(int family, int degree) {
    switch (family) {
        case EXPFAM_BERNOULLI: return 3;
        case EXPFAM_COUNTS: return 2 + degree;
        case EXPFAM_ONEHOT: return 1 + degree;
        case EXPFAM_POISSON: return 3;
        case EXPFAM_EXPONENTIAL: return 2;
        default: return 4;
    }
}

// The checks every entry point shares; `ints` says which dtypes the family reads.
static int check_common(const char* who, bool ints, int dtype, const void* x, int64_t n, const void* stats, const void* work) {
    if (dtype < EXPFAM_U8 || dtype > EXPFAM_F64) return g_err.fail(EXPFAM_EINVAL, "%s: dtype must be an expfam_dtype", who);
    if (ints ? !is_int_dtype(dtype) : !is_float_dtype(dtype))
        return g_err.fail(EXPFAM_EINVAL, "%s: dtype must be %s", who,
                          ints ? "EXPFAM_U8, EXPFAM_I32 or EXPFAM_I64" : "EXPFAM_F32 or EXPFAM_F64");
    if (n < 1) return g_err.fail(EXPFAM_EINVAL, "%s: n must be >= 1", who);
    if (!x || !stats || !work) return g_err.fail(EXPFAM_EINVAL, "%s: null pointer", who);
    if (misaligned(x, elem_size(dtype))) return g_err.fail(EXPFAM_EINVAL, "%s: x_dev must be aligned to its element size", who);
    return EXPFAM_OK;
}

static int check_degree(const char* who, int degree) {
    if (degree < 1) return g_err.fail(EXPFAM_EINVAL, "%s: degree must be >= 1", who);
    if (degree > EXPFAM_MAX_DEGREE)
        return g_err.fail(EXPFAM_EUNSUPPORTED, "%s: degree > %d is not supported", who, EXPFAM_MAX_DEGREE);
    return EXPFAM_OK;
}

// Ranges of whole 16-byte vectors, the same for the same pointer alignment and n (run-to-run identical sums).
template <typename T, typename ACC>
static int launch_stream(const void* x_dev, int64_t n, int degree, int max_slot, int dsum_slot, bool normal, void* stats_dev,
                         void* work_dev, hipStream_t st) {
    constexpr int V = 16 / sizeof(T);
    const T* x = (const T*)x_dev;
    int64_t head = (int64_t)(((16 - (uintptr_t)x % 16) % 16) / sizeof(T));
    if (head > n) head = n;
    const int64_t nvec = (n - head) / V;
    int64_t vps = (nvec + kMaxSlabs - 1) / kMaxSlabs;
    if (vps < kMinVecs) vps = kMinVecs;
    const int S = nvec > 0 ? (int)((nvec + vps - 1) / vps) : 1;
    const int len = ACC::slab_len(degree);
    hipLaunchKernelGGL((stream_kernel<T, ACC>), dim3(S), dim3(kThreads), ACC::lds_bytes(degree), st, x, n, head, nvec, vps,
                       degree, (int64_t*)work_dev);
    if (int rc = g_err.launched("stream_kernel launch")) return rc;
    if (normal) {
        hipLaunchKernelGGL(combine_normal_kernel, dim3(1), dim3(64), 0, st, (const int64_t*)work_dev, S, n, (int64_t*)stats_dev);
        return g_err.launched("combine_normal_kernel launch");
    }
    hipLaunchKernelGGL(combine_kernel, dim3(grid_of(len, kThreads)), dim3(kThreads), 0, st, (const int64_t*)work_dev,
                       S, len, n, max_slot, dsum_slot, (int64_t*)stats_dev);
    return g_err.launched("combine_kernel launch");
}

template <template <typename> class ACC>
static int launch_ints(int dtype, const void* x, int64_t n, int dsum_slot, void* stats, void* work, hipStream_t st) {
    if (dtype == EXPFAM_U8) return launch_stream<uint8_t, ACC<uint8_t>>(x, n, 0, -1, dsum_slot, false, stats, work, st);
    if (dtype == EXPFAM_I32) return launch_stream<int32_t, ACC<int32_t>>(x, n, 0, -1, dsum_slot, false, stats, work, st);
    return launch_stream<int64_t, ACC<int64_t>>(x, n, 0, -1, dsum_slot, false, stats, work, st);
}

template <typename T>
static int launch_counts(const void* x, int64_t n, int degree, void* stats, void* work, hipStream_t st) {
    if (degree <= kRegBins) return launch_stream<T, CountsAcc<T, true>>(x, n, degree, 1, -1, false, stats, work, st);
    return launch_stream<T, CountsAcc<T, false>>(x, n, degree, 1, -1, false, stats, work, st);
}

template <typename T>
static int launch_onehot(const void* x_dev, int64_t n, int degree, int64_t ld, void* stats_dev, void* work_dev, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const int blocks = (degree + V - 1) / V;        // 16-byte blocks of an aligned row
    int W = 1;
    while (W < blocks && W < 64) W <<= 1;
    // rows per workgroup: whole unrolled wave steps, at least 32 KiB of the sample, at most kMaxSlabs ranges
    const int64_t step = (int64_t)kWaves * (64 / W) * kUnroll;
    int64_t rps = (n + kMaxSlabs - 1) / kMaxSlabs;
    const int64_t min_rows = (int64_t)(16 * kMinVecs) / ((int64_t)degree * (int64_t)sizeof(T)) + 1;
    if (rps < min_rows) rps = min_rows;
    rps = (rps + step - 1) / step * step;
    const int S = (int)((n + rps - 1) / rps);
    hipLaunchKernelGGL((onehot_kernel<T>), dim3(S), dim3(kThreads), sizeof(unsigned long long) * (size_t)degree, st,
                       (const T*)x_dev, n, degree, ld, W, rps, (int64_t*)work_dev);
    if (int rc = g_err.launched("onehot_kernel launch")) return rc;
    const int len = 1 + degree;
    hipLaunchKernelGGL(combine_kernel, dim3(grid_of(len, kThreads)), dim3(kThreads), 0, st, (const int64_t*)work_dev,
                       S, len, n, -1, -1, (int64_t*)stats_dev);
    return g_err.launched("combine_kernel launch");
}
}  // namespace expfam

using namespace expfam;

extern "C" {

int expfam_abi_version(void) { return EXPFAM_ABI_VERSION; }
const char* expfam_last_error(void) { return g_err.msg; }

int64_t expfam_stats_len(int family, int degree) {
    if (family < EXPFAM_BERNOULLI || family > EXPFAM_NORMAL) return -1;
    if (has_degree(family) && (degree < 1 || degree > EXPFAM_MAX_DEGREE)) return -1;
    return family == EXPFAM_NORMAL ? 3 : 1 + slab_len(family, degree);
}

int64_t expfam_work_len(int family, int degree) {
    if (family < EXPFAM_BERNOULLI || family > EXPFAM_NORMAL) return -1;
    if (has_degree(family) && (degree < 1 || degree > EXPFAM_MAX_DEGREE)) return -1;
    return (int64_t)kMaxSlabs * slab_len(family, degree);
}

int expfam_stats_bernoulli(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expfam_stats_bernoulli", true, dtype, x_dev, n, stats_dev, work_dev)) return rc;
    return launch_ints<BernoulliAcc>(dtype, x_dev, n, -1, stats_dev, work_dev, (hipStream_t)stream);
}

int expfam_stats_counts(int dtype, const void* x_dev, int64_t n, int degree, void* stats_dev, void* work_dev, void* stream) {
    if (int rc = check_degree("expfam_stats_counts", degree)) return rc;
    if (int rc = check_common("expfam_stats_counts", true, dtype, x_dev, n, stats_dev, work_dev)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EXPFAM_U8) return launch_counts<uint8_t>(x_dev, n, degree, stats_dev, work_dev, st);
    if (dtype == EXPFAM_I32) return launch_counts<int32_t>(x_dev, n, degree, stats_dev, work_dev, st);
    return launch_counts<int64_t>(x_dev, n, degree, stats_dev, work_dev, st);
}

int expfam_stats_onehot(int dtype, const void* x_dev, int64_t n, int degree, int64_t ld, void* stats_dev, void* work_dev,
                        void* stream) {
    if (int rc = check_degree("expfam_stats_onehot", degree)) return rc;
    if (int rc = check_common("expfam_stats_onehot", true, dtype, x_dev, n, stats_dev, work_dev)) return rc;
    if (ld < degree) return g_err.fail(EXPFAM_EINVAL, "expfam_stats_onehot: ld must be >= degree");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EXPFAM_U8) return launch_onehot<uint8_t>(x_dev, n, degree, ld, stats_dev, work_dev, st);
    if (dtype == EXPFAM_I32) return launch_onehot<int32_t>(x_dev, n, degree, ld, stats_dev, work_dev, st);
    return launch_onehot<int64_t>(x_dev, n, degree, ld, stats_dev, work_dev, st);
}

int expfam_stats_poisson(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expfam_stats_poisson", true, dtype, x_dev, n, stats_dev, work_dev)) return rc;
    return launch_ints<PoissonAcc>(dtype, x_dev, n, 2, stats_dev, work_dev, (hipStream_t)stream);
}

int expfam_stats_exponential(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expfam_stats_exponential", false, dtype, x_dev, n, stats_dev, work_dev)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EXPFAM_F32)
        return launch_stream<float, ExponentialAcc<float>>(x_dev, n, 0, -1, 1, false, stats_dev, work_dev, st);
    return launch_stream<double, ExponentialAcc<double>>(x_dev, n, 0, -1, 1, false, stats_dev, work_dev, st);
}

int expfam_stats_normal(int dtype, const void* x_dev, int64_t n, void* stats_dev, void* work_dev, void* stream) {
    if (int rc = check_common("expfam_stats_normal", false, dtype, x_dev, n, stats_dev, work_dev)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EXPFAM_F32) return launch_stream<float, NormalAcc<float>>(x_dev, n, 0, -1, -1, true, stats_dev, work_dev, st);
    return launch_stream<double, NormalAcc<double>>(x_dev, n, 0, -1, -1, true, stats_dev, work_dev, st);
}

}  // extern "C"
