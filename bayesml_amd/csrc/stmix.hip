// include/stmix.h: the argument checks and the launches of stmix_kernels.h.
#include "../../include/stmix.h"
#include "entry.h"
#include "stmix_kernels.h"

namespace stmix {
ENTRY_SAME_CODES(STMIX);
static_assert(STMIX_MAX_DEGREE == 19200, "generic_rows (generic.h) holds one row of up to 19200 doubles in LDS");
static thread_local entry::Err g_err = {""};

static const char* check_shape(int K, int D) {
    if (K < 1 || K > STMIX_MAX_COMPONENTS) return "K must be in 1..65536";
    if (D < 1 || D > STMIX_MAX_DEGREE) return "D must be in 1..19200";
    return nullptr;
}

struct Args {
    int K, D;
    int64_t ldx, n_rows;
    const double *pivot, *img, *c, *nu;
    double* lnp;
    int64_t* z;
    hipStream_t st;
};

template <int T, typename XT>
static void launch_fused_t(const XT* x, bool vec, const Args& a) {
    constexpr int rows_per_wg = kWaves * 16 * estep_nb_w<double>(T, kWaves);
    int64_t grid = (a.n_rows + rows_per_wg - 1) / rows_per_wg;
    if (grid > (1 << 20)) grid = 1 << 20;
    if (vec)
        hipLaunchKernelGGL((fused_kernel<T, XT, true>), dim3((unsigned)grid), dim3(64 * kWaves), 0, a.st, x, a.ldx, a.n_rows, a.D,
                           a.pivot, a.img, a.c, a.nu, a.K, a.lnp, a.z);
    else
        hipLaunchKernelGGL((fused_kernel<T, XT, false>), dim3((unsigned)grid), dim3(64 * kWaves), 0, a.st, x, a.ldx, a.n_rows,
                           a.D, a.pivot, a.img, a.c, a.nu, a.K, a.lnp, a.z);
}

template <typename XT>
static int launch_fused(const XT* x, bool vec, const Args& a) {
    switch ((a.D + 15) / 16) {
        case 1: launch_fused_t<1>(x, vec, a); break;
        case 2: launch_fused_t<2>(x, vec, a); break;
        case 3: launch_fused_t<3>(x, vec, a); break;
        case 4: launch_fused_t<4>(x, vec, a); break;
        case 5: launch_fused_t<5>(x, vec, a); break;
        case 6: launch_fused_t<6>(x, vec, a); break;
        case 7: launch_fused_t<7>(x, vec, a); break;
        default: launch_fused_t<8>(x, vec, a); break;
    }
    return g_err.launched("stmix fused_kernel launch");
}

template <typename XT>
static int launch_plain(const XT* x, const Args& a) {
    const int R = gmmvb::generic_rows(a.D);
    const int lds = (int)((size_t)a.D * R * sizeof(double));
    const hipError_t e = hipFuncSetAttribute((const void*)plain_kernel<XT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return g_err.hip(STMIX_EHIP, "stmix plain_kernel attribute", e);
    int64_t grid = (a.n_rows + R - 1) / R;
    if (grid > (1 << 20)) grid = 1 << 20;
    hipLaunchKernelGGL(plain_kernel<XT>, dim3((unsigned)grid), dim3(64), (size_t)lds, a.st, x, a.ldx, a.n_rows, a.D, a.pivot, a.img,
                       a.c, a.nu, a.K, R, a.lnp, a.z);
    return g_err.launched("stmix plain_kernel launch");
}
}  // namespace stmix

using namespace stmix;

extern "C" {

int stmix_abi_version(void) { return STMIX_ABI_VERSION; }
const char* stmix_last_error(void) { return g_err.msg; }

int64_t stmix_image_len(int K, int D) { return check_shape(K, D) ? -1 : (int64_t)K * image_doubles(D); }

int stmix_pack(int K, int D, const double* u_dev, const double* m_dev, const double* pivot_dev, double* img_dev,
               void* stream) {
    const char* who = "stmix_pack";
    if (const char* bad = check_shape(K, D)) return g_err.fail(STMIX_EINVAL, "%s: %s", who, bad);
    if (!u_dev || !m_dev || !pivot_dev || !img_dev) return g_err.fail(STMIX_EINVAL, "%s: null pointer", who);
    if (entry::any_misaligned(8, u_dev, m_dev, pivot_dev)) return g_err.fail(STMIX_EINVAL, "%s: the double arrays must be 8-byte aligned", who);
    if (entry::misaligned(img_dev, 16)) return g_err.fail(STMIX_EINVAL, "%s: img_dev must be 16-byte aligned", who);
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, u_dev, m_dev, pivot_dev, D, img_dev);
    return g_err.launched("stmix pack_kernel launch");
}

int stmix_logpdf(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* pivot_dev,
                 const double* img_dev, const double* c_dev, const double* nu_dev, double* lnp_dev, int64_t* z_dev,
                 void* stream) {
    const char* who = "stmix_logpdf";
    if (const char* bad = check_shape(K, D)) return g_err.fail(STMIX_EINVAL, "%s: %s", who, bad);
    if (x_dtype != STMIX_F32 && x_dtype != STMIX_F64)
        return g_err.fail(STMIX_EINVAL, "%s: x_dtype must be STMIX_F32 or STMIX_F64", who);
    if (n_rows < 1) return g_err.fail(STMIX_EINVAL, "%s: n_rows must be >= 1", who);
    if (ldx < D) return g_err.fail(STMIX_EINVAL, "%s: ldx must be >= D", who);
    if (!x_dev || !pivot_dev || !img_dev || !c_dev || !nu_dev || !lnp_dev) return g_err.fail(STMIX_EINVAL, "%s: null pointer", who);
    const size_t esz = x_dtype == STMIX_F32 ? 4 : 8;
    if (entry::misaligned(x_dev, esz)) return g_err.fail(STMIX_EINVAL, "%s: x must be aligned to its element size", who);
    if (entry::any_misaligned(8, pivot_dev, c_dev, nu_dev, lnp_dev) || entry::misaligned(z_dev, 8))
        return g_err.fail(STMIX_EINVAL, "%s: the double and int64 arrays must be 8-byte aligned", who);
    if (entry::misaligned(img_dev, 16)) return g_err.fail(STMIX_EINVAL, "%s: img_dev must be 16-byte aligned", who);
    const Args a = {K, D, ldx, n_rows, pivot_dev, img_dev, c_dev, nu_dev, lnp_dev, z_dev, (hipStream_t)stream};
    if (D > 128) return x_dtype == STMIX_F32 ? launch_plain((const float*)x_dev, a) : launch_plain((const double*)x_dev, a);
    // vector loads: whole 16-feature blocks, 4-element vectors naturally aligned
    const bool vec = D % 16 == 0 && (uintptr_t)x_dev % (4 * esz) == 0 && ldx % 4 == 0;
    return x_dtype == STMIX_F32 ? launch_fused((const float*)x_dev, vec, a) : launch_fused((const double*)x_dev, vec, a);
}

}  // extern "C"
