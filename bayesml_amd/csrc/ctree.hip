// include/ctree.h: argument checks, the layout of the level tables and of the scratch, and the launches of ctree_kernels.h.
#include "../../include/ctree.h"
#include "ctree_kernels.h"
#include "ctree_shape.h"

namespace ctree {
using namespace entry;
using namespace ctree_shape;
ENTRY_SAME_CODES(CTREE);
static thread_local Err g_err = {""};

static int check_shape(const char* who, int k, int D, Shape* sh) {
    const int rc = shape_of(k, D, sh);
    if (rc == CTREE_EINVAL) return g_err.fail(rc, "%s: k and D must be >= 1", who);
    if (rc == CTREE_EUNSUPPORTED)
        return g_err.fail(rc, "%s: k > %d or k^(D+1) > %d is not supported", who, CTREE_MAX_K, CTREE_MAX_SLOTS);
    return CTREE_OK;
}

static bool lds_path(const Shape& sh) { return sh.bins <= CTREE_LDS_BINS; }
static int64_t count_work(const Shape& sh) { return (int64_t)kMaxSlabs * (lds_path(sh) ? 1 + sh.bins : 1); }
// scratch: [ count slabs | lnW or MAP value, all levels | counts of levels 0..D-1 ]
static double* level_values(const Shape& sh, void* work) { return (double*)work + count_work(sh); }
static int64_t* level_counts(const Shape& sh, void* work) { return (int64_t*)work + count_work(sh) + sh.nodes; }

static int elem_size(int d) { return d == CTREE_U8 ? 1 : d == CTREE_I32 ? 4 : 8; }

template <typename T>
static int launch_count(const void* x_dev, int64_t n, int k, int D, const Shape& sh, void* out_dev, void* work_dev,
                        hipStream_t st) {
    int64_t span;
    const int S = slab_span(n, kMaxSlabs, kMinSpan, &span);
    int64_t* out = (int64_t*)out_dev;
    if (lds_path(sh)) {
        hipLaunchKernelGGL((count_kernel<T, true>), dim3(S), dim3(kThreads), sizeof(unsigned long long) * (size_t)sh.bins, st,
                           (const T*)x_dev, n, span, k, D, sh.bins, (unsigned long long*)nullptr, (int64_t*)work_dev);
        if (int rc = g_err.launched("count_kernel launch")) return rc;
        hipLaunchKernelGGL(count_combine_kernel, dim3(grid_of(1 + sh.bins, kThreads)), dim3(kThreads), 0, st,
                           (const int64_t*)work_dev, S, 1 + sh.bins, n, out);
        return g_err.launched("count_combine_kernel launch");
    }
    const hipError_t e = hipMemsetAsync(out + 2, 0, sizeof(int64_t) * (size_t)sh.bins, st);
    if (e != hipSuccess) return g_err.hip(CTREE_EHIP, "ctree_count: hipMemsetAsync", e);
    hipLaunchKernelGGL((count_kernel<T, false>), dim3(S), dim3(kThreads), 0, st, (const T*)x_dev, n, span, k, D, sh.bins,
                       (unsigned long long*)(out + 2), (int64_t*)work_dev);
    if (int rc = g_err.launched("count_kernel launch")) return rc;
    hipLaunchKernelGGL(count_combine_kernel, dim3(1), dim3(kThreads), 0, st, (const int64_t*)work_dev, S, (int64_t)1, n, out);
    return g_err.launched("count_combine_kernel launch");
}
}  // namespace ctree

using namespace ctree;

extern "C" {

int ctree_abi_version(void) { return CTREE_ABI_VERSION; }
const char* ctree_last_error(void) { return g_err.msg; }

int64_t ctree_table_len(int k, int D, int level) {
    Shape sh;
    if (shape_of(k, D, &sh) != CTREE_OK || level < -1 || level > D) return -1;
    return level < 0 ? sh.nodes : sh.pw[level];
}

int64_t ctree_work_len(int k, int D) {
    Shape sh;
    if (shape_of(k, D, &sh) != CTREE_OK) return -1;
    return count_work(sh) + sh.nodes + sh.upper * k;
}

int ctree_count(int dtype, const void* x_dev, int64_t n, int k, int D, void* out_dev, void* work_dev, void* stream) {
    Shape sh;
    if (int rc = check_shape("ctree_count", k, D, &sh)) return rc;
    if (dtype < CTREE_U8 || dtype > CTREE_I64)
        return g_err.fail(CTREE_EINVAL, "ctree_count: dtype must be CTREE_U8, CTREE_I32 or CTREE_I64");
    if (n < 1) return g_err.fail(CTREE_EINVAL, "ctree_count: n must be >= 1");
    if (!x_dev || !out_dev || !work_dev) return g_err.fail(CTREE_EINVAL, "ctree_count: null pointer");
    if (misaligned(x_dev, elem_size(dtype)))
        return g_err.fail(CTREE_EINVAL, "ctree_count: x_dev must be aligned to its element size");
    if (any_misaligned(8, out_dev, work_dev))
        return g_err.fail(CTREE_EINVAL, "ctree_count: out_dev and work_dev must be aligned to 8 bytes");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CTREE_U8) return launch_count<uint8_t>(x_dev, n, k, D, sh, out_dev, work_dev, st);
    if (dtype == CTREE_I32) return launch_count<int32_t>(x_dev, n, k, D, sh, out_dev, work_dev, st);
    return launch_count<int64_t>(x_dev, n, k, D, sh, out_dev, work_dev, st);
}

int ctree_sweep(int k, int D, const void* cnt_dev, const void* head_dev, int n_head, void* beta_dev, void* g_dev,
                void* exists_dev, double hn_g, const void* hn_beta_dev, void* cnt_levels_dev, void* work_dev, void* stream) {
    Shape sh;
    if (int rc = check_shape("ctree_sweep", k, D, &sh)) return rc;
    if (n_head < 0 || n_head > D) return g_err.fail(CTREE_EINVAL, "ctree_sweep: n_head must be in 0..D");
    if (!cnt_dev || !beta_dev || !g_dev || !exists_dev || !hn_beta_dev || !work_dev || (n_head > 0 && !head_dev))
        return g_err.fail(CTREE_EINVAL, "ctree_sweep: null pointer");
    if (!(hn_g >= 0.0 && hn_g <= 1.0)) return g_err.fail(CTREE_EINVAL, "ctree_sweep: hn_g must be in [0, 1]");
    if (any_misaligned(8, cnt_dev, beta_dev, g_dev, hn_beta_dev, cnt_levels_dev, work_dev) || misaligned(head_dev, 4))
        return g_err.fail(CTREE_EINVAL, "ctree_sweep: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    double* lnw = level_values(sh, work_dev);
    int64_t* cl = cnt_levels_dev ? (int64_t*)cnt_levels_dev : level_counts(sh, work_dev);
    double* beta = (double*)beta_dev;
    double* g = (double*)g_dev;
    uint8_t* ex = (uint8_t*)exists_dev;
    const double* hb = (const double*)hn_beta_dev;
    hipLaunchKernelGGL(sweep_deepest_kernel, dim3(grid_of(sh.pw[D], kThreads)), dim3(kThreads), 0, st, k, sh.pw[D],
                       (const int64_t*)cnt_dev, beta + sh.off[D] * k, g + sh.off[D], ex + sh.off[D], hb, lnw + sh.off[D]);
    if (int rc = g_err.launched("sweep_deepest_kernel launch")) return rc;
    for (int d = D - 1; d >= 0; --d) {
        const int64_t* child = d + 1 == D ? (const int64_t*)cnt_dev : cl + sh.off[d + 1] * k;
        hipLaunchKernelGGL(sweep_level_kernel, dim3(grid_of(sh.pw[d], kThreads)), dim3(kThreads), 0, st, k, d, sh.pw[d], child,
                           cl + sh.off[d] * k, (const double*)(lnw + sh.off[d + 1]), lnw + sh.off[d], beta + sh.off[d] * k,
                           g + sh.off[d], ex + sh.off[d], hn_g, hb, (const int32_t*)head_dev, n_head);
        if (int rc = g_err.launched("sweep_level_kernel launch")) return rc;
    }
    return CTREE_OK;
}

int ctree_map(int k, int D, const void* g_dev, const void* exists_dev, double hn_g, void* map_leaf_dev, void* work_dev,
              void* stream) {
    Shape sh;
    if (int rc = check_shape("ctree_map", k, D, &sh)) return rc;
    if (!g_dev || !exists_dev || !map_leaf_dev || !work_dev) return g_err.fail(CTREE_EINVAL, "ctree_map: null pointer");
    if (!(hn_g >= 0.0 && hn_g <= 1.0)) return g_err.fail(CTREE_EINVAL, "ctree_map: hn_g must be in [0, 1]");
    if (any_misaligned(8, g_dev, work_dev)) return g_err.fail(CTREE_EINVAL, "ctree_map: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    double* val = level_values(sh, work_dev);
    const double* g = (const double*)g_dev;
    const uint8_t* ex = (const uint8_t*)exists_dev;
    uint8_t* ml = (uint8_t*)map_leaf_dev;
    for (int d = D; d >= 0; --d) {
        const double pw_here = d < D ? subtree_pow(hn_g, k, D, d) : 1.0;
        const double pw_parent = d > 0 ? subtree_pow(hn_g, k, D, d - 1) : 1.0;
        // (the neighbouring levels' pointers are not read at d = D and d = 0; they point at this level's tables there)
        const int dc = d < D ? d + 1 : d, dp = d > 0 ? d - 1 : d;
        hipLaunchKernelGGL(map_level_kernel, dim3(grid_of(sh.pw[d], kThreads)), dim3(kThreads), 0, st, k, d, D, sh.pw[d],
                           g + sh.off[d], ex + sh.off[d], ex + sh.off[dc], (const double*)(val + sh.off[dc]), g + sh.off[dp],
                           ex + sh.off[dp], pw_here, pw_parent, val + sh.off[d], ml + sh.off[d]);
        if (int rc = g_err.launched("map_level_kernel launch")) return rc;
    }
    return CTREE_OK;
}

}  // extern "C"
