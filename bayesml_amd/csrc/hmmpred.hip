// include/hmmpred.h: the argument checks, the plan of a call and the launches of hmmpred_kernels.h.
//
// hmm.h and hmm_generic.h define their non-template kernels with external linkage, and hmm_capi.o already holds them: this
// object compiles the headers under a namespace of its own, so the two sets of host stubs do not meet at link time.
#define gmmvb gmmvb_hmmpred
#include "../../include/hmmpred.h"
#include "../../include/stmix.h"
#include "entry.h"
#include "hmmpred_kernels.h"

#include <type_traits>

namespace hmmpred {
ENTRY_SAME_CODES(HMMPRED);
static_assert(HMMPRED_MAX_DEGREE == STMIX_MAX_DEGREE, "the parameter image is stmix_pack's");
static_assert(HMMPRED_MAX_STATES == kWalkThreads, "walk_kernel: a thread per state");
static_assert(HMMPRED_PARALLEL_STATES == 64, "hmm.h: KT <= 4 blocks of 16 states");
static thread_local entry::Err g_err = {""};

// hmm_capi.hip's kHmmForgetTol, kHmmShortForgetFrom / kHmmShortChunk, kHmmLongFrom / kHmmLongChunk and sweep_len
constexpr double kForgetTol = 2e-13;
constexpr int64_t kShortFrom = 4096, kShortChunk = 32, kLongFrom = int64_t(1) << 15, kLongChunk = 256, kSweep = 64;
constexpr int kCheckBlocks = 1024;

// The scratch of a call, in doubles from its start.  ln e [K][npad] lies where phi will: hmm_prep_kernel has consumed it
// before the recursion writes a row.
struct Layout {
    int Kp;
    int64_t npad, chunk_cap;
    int64_t rho, phi, s, m, starts, ends, gate, total;
};
static Layout layout(int K, int64_t n_rows) {
    Layout l;
    l.Kp = 16 * ((K + 15) / 16);
    l.npad = (n_rows + 63) / 64 * 64;
    l.chunk_cap = (n_rows - 1 + HMMPRED_MIN_CHUNK - 1) / HMMPRED_MIN_CHUNK + 1;
    l.rho = 0;
    l.phi = l.rho + l.npad * l.Kp;
    l.s = l.phi + l.npad * l.Kp;
    l.m = l.s + l.npad;
    l.starts = l.m + l.npad;
    l.ends = l.starts + l.chunk_cap * l.Kp;
    l.gate = l.ends + l.chunk_cap * l.Kp;
    l.total = l.gate + 2;
    return l;
}

static const char* check_shape(int K, int D, int64_t n_rows) {
    if (K < 1) return "K must be >= 1";
    if (D < 1 || D > HMMPRED_MAX_DEGREE) return "D must be in 1..19200";
    if (n_rows < 1) return "n_rows must be >= 1";
    return nullptr;
}

struct Args {
    int K, D;
    int64_t ldx, n_rows;
    const double *pivot, *img, *c, *nu;
    double* lne;
    int64_t npad;
    hipStream_t st;
};

template <int T, typename XT>
static void launch_emission_t(const XT* x, bool vec, const Args& a) {
    constexpr int rows_per_wg = kWaves * 16 * estep_nb_w<double>(T, kWaves);
    int64_t grid = (a.n_rows + rows_per_wg - 1) / rows_per_wg;
    if (grid > (1 << 20)) grid = 1 << 20;
    if (vec)
        hipLaunchKernelGGL((emission_kernel<T, XT, true>), dim3((unsigned)grid), dim3(64 * kWaves), 0, a.st, x, a.ldx, a.n_rows,
                           a.D, a.pivot, a.img, a.c, a.nu, a.K, a.lne, a.npad);
    else
        hipLaunchKernelGGL((emission_kernel<T, XT, false>), dim3((unsigned)grid), dim3(64 * kWaves), 0, a.st, x, a.ldx, a.n_rows,
                           a.D, a.pivot, a.img, a.c, a.nu, a.K, a.lne, a.npad);
}

template <typename XT>
static int launch_emission(const XT* x, bool vec, const Args& a) {
    switch ((a.D + 15) / 16) {
        case 1: launch_emission_t<1>(x, vec, a); break;
        case 2: launch_emission_t<2>(x, vec, a); break;
        case 3: launch_emission_t<3>(x, vec, a); break;
        case 4: launch_emission_t<4>(x, vec, a); break;
        case 5: launch_emission_t<5>(x, vec, a); break;
        case 6: launch_emission_t<6>(x, vec, a); break;
        case 7: launch_emission_t<7>(x, vec, a); break;
        default: launch_emission_t<8>(x, vec, a); break;
    }
    return g_err.launched("hmmpred emission_kernel launch");
}

template <typename XT>
static int launch_emission_plain(const XT* x, const Args& a) {
    const int R = gmmvb::generic_rows(a.D);
    const int lds = (int)((size_t)a.D * R * sizeof(double));
    const hipError_t e =
        hipFuncSetAttribute((const void*)emission_plain_kernel<XT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return g_err.hip(HMMPRED_EHIP, "hmmpred emission_plain_kernel attribute", e);
    int64_t grid = (a.n_rows + R - 1) / R;
    if (grid > (1 << 20)) grid = 1 << 20;
    hipLaunchKernelGGL(emission_plain_kernel<XT>, dim3((unsigned)grid), dim3(64), (size_t)lds, a.st, x, a.ldx, a.n_rows, a.D,
                       a.pivot, a.img, a.c, a.nu, a.K, R, a.lne, a.npad);
    return g_err.launched("hmmpred emission_plain_kernel launch");
}

// sweep, replay and check of the chunk-parallel filter for KT blocks of 16 states
template <int KT>
static void launch_parallel(const double* rho, const double* a, int K, int64_t T, int64_t L, int64_t W, int64_t n_chunks,
                            double* starts, double* ends, double* phi, double* s, int* gate, hipStream_t st) {
    const unsigned grid = (unsigned)((n_chunks + 4 * gmmvb::kReplayChunks - 1) / (4 * gmmvb::kReplayChunks));
    hipLaunchKernelGGL((sweep_kernel<KT>), dim3(grid), dim3(256), 0, st, rho, a, K, T, L, n_chunks, starts, W);
    hipLaunchKernelGGL((gmmvb::hmm_forward_replay_kernel<KT>), dim3(grid), dim3(256), 0, st, rho, a, K, T, L, n_chunks,
                       (const double*)starts, phi, s, 0, ends, (const int*)nullptr);
    const int64_t n = (n_chunks - 1) * 16 * KT;
    const unsigned cgrid = (unsigned)std::min<int64_t>(kCheckBlocks, (n + 255) / 256);
    // (the kernel tests a forward and a backward pair of arrays: the one pair there is here is handed in as both)
    hipLaunchKernelGGL(gmmvb::hmm_boundary_check_kernel<true>, dim3(cgrid), dim3(256), 0, st, (const double*)starts,
                       (const double*)ends, (const double*)starts + 16 * KT, (const double*)ends + 16 * KT, n, 16 * KT,
                       kForgetTol, gate, (const int*)nullptr);
}
}  // namespace hmmpred

using namespace hmmpred;

extern "C" {

int hmmpred_abi_version(void) { return HMMPRED_ABI_VERSION; }
const char* hmmpred_last_error(void) { return g_err.msg; }

int64_t hmmpred_scratch_len(int K, int D, int64_t n_rows) {
    if (check_shape(K, D, n_rows) || K > HMMPRED_MAX_STATES) return -1;
    return layout(K, n_rows).total;
}

int hmmpred_logpdf(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, const double* pivot_dev,
                   const double* img_dev, const double* c_dev, const double* nu_dev, const double* a_dev,
                   const double* w0_dev, int64_t chunk_len, int64_t sweep_len, double* scratch_dev, double* lnp_dev,
                   int64_t* z_dev, double* end_dev, int64_t* diag_dev, void* stream) {
    const char* who = "hmmpred_logpdf";
    if (const char* bad = check_shape(K, D, n_rows)) return g_err.fail(HMMPRED_EINVAL, "%s: %s", who, bad);
    if (K > HMMPRED_MAX_STATES)
        return g_err.fail(HMMPRED_EUNSUPPORTED, "%s: at most %d states in this version (got %d)", who, HMMPRED_MAX_STATES, K);
    if (x_dtype != HMMPRED_F32 && x_dtype != HMMPRED_F64)
        return g_err.fail(HMMPRED_EINVAL, "%s: x_dtype must be HMMPRED_F32 or HMMPRED_F64", who);
    if (ldx < D) return g_err.fail(HMMPRED_EINVAL, "%s: ldx must be >= D", who);
    if (chunk_len != 0 && chunk_len < HMMPRED_MIN_CHUNK)
        return g_err.fail(HMMPRED_EINVAL, "%s: chunk_len must be 0 or >= %d", who, HMMPRED_MIN_CHUNK);
    if (sweep_len < 0) return g_err.fail(HMMPRED_EINVAL, "%s: sweep_len must be >= 0", who);
    if (!x_dev || !pivot_dev || !img_dev || !c_dev || !nu_dev || !a_dev || !w0_dev || !scratch_dev || !lnp_dev || !end_dev ||
        !diag_dev)
        return g_err.fail(HMMPRED_EINVAL, "%s: null pointer", who);
    const size_t esz = x_dtype == HMMPRED_F32 ? 4 : 8;
    if (entry::misaligned(x_dev, esz)) return g_err.fail(HMMPRED_EINVAL, "%s: x must be aligned to its element size", who);
    if (entry::any_misaligned(8, pivot_dev, c_dev, nu_dev, a_dev, w0_dev, lnp_dev, end_dev) || entry::misaligned(z_dev, 8) ||
        entry::misaligned(diag_dev, 8))
        return g_err.fail(HMMPRED_EINVAL, "%s: the double and int64 arrays must be 8-byte aligned", who);
    if (entry::misaligned(img_dev, 16) || entry::misaligned(scratch_dev, 16))
        return g_err.fail(HMMPRED_EINVAL, "%s: img_dev and scratch_dev must be 16-byte aligned", who);

    const hipStream_t st = (hipStream_t)stream;
    const int64_t T = n_rows;
    const Layout l = layout(K, T);
    const int Kp = l.Kp;
    double* const rho = scratch_dev + l.rho;
    double* const phi = scratch_dev + l.phi;
    double* const lne = phi;
    double* const s = scratch_dev + l.s;
    double* const m = scratch_dev + l.m;
    double* const starts = scratch_dev + l.starts;
    double* const ends = scratch_dev + l.ends;
    int* const gate = reinterpret_cast<int*>(scratch_dev + l.gate);

    // the plan: chunk-parallel from two chunks on and up to 64 states, one serial walk otherwise
    int64_t L = chunk_len != 0 ? chunk_len : (T < kShortFrom ? 0 : (T > kLongFrom ? kLongChunk : kShortChunk));
    int64_t W = sweep_len != 0 ? sweep_len : kSweep;
    int64_t n_chunks = L > 0 ? (T - 1 + L - 1) / L : 0;
    const bool parallel = K <= HMMPRED_PARALLEL_STATES && n_chunks >= 2;
    if (!parallel) {
        L = T;
        n_chunks = T > 1 ? 1 : 0;
    }
    if (W > L) W = L;

    // 1. emission: ln e component-major, then rho' (lane order) and m
    const Args a = {K, D, ldx, T, pivot_dev, img_dev, c_dev, nu_dev, lne, l.npad, st};
    int rc;
    if (D > 128) {
        rc = x_dtype == HMMPRED_F32 ? launch_emission_plain((const float*)x_dev, a) : launch_emission_plain((const double*)x_dev, a);
    } else {
        const bool vec = D % 16 == 0 && (uintptr_t)x_dev % (4 * esz) == 0 && ldx % 4 == 0;
        rc = x_dtype == HMMPRED_F32 ? launch_emission((const float*)x_dev, vec, a) : launch_emission((const double*)x_dev, vec, a);
    }
    if (rc != HMMPRED_OK) return rc;
    const unsigned pgrid = (unsigned)((T + gmmvb::kPrepSteps - 1) / gmmvb::kPrepSteps);
    if (K <= 64)
        hipLaunchKernelGGL(gmmvb::hmm_prep_kernel, dim3(pgrid), dim3(256),
                           ((size_t)Kp * (gmmvb::kPrepSteps + 1) + gmmvb::kPrepSteps) * sizeof(double), st, (const double*)lne, l.npad,
                           T, K, Kp, rho, m);
    else
        hipLaunchKernelGGL(gmmvb::hmm_prep_generic_kernel, dim3(pgrid), dim3(256), 0, st, (const double*)lne, l.npad, T, K, Kp, rho,
                           m);
    if ((rc = g_err.launched("hmmpred prep launch")) != HMMPRED_OK) return rc;

    // 2. the filter
    hipLaunchKernelGGL(first_step_kernel, dim3(1), dim3(kWalkThreads), 0, st, (const double*)rho, w0_dev, K, Kp, phi, s, starts, gate,
                       diag_dev);
    if (parallel) {
        auto go = [&](auto kt) {
            launch_parallel<decltype(kt)::value>(rho, a_dev, K, T, L, W, n_chunks, starts, ends, phi, s, gate, st);
        };
        switch (Kp / 16) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 3: go(std::integral_constant<int, 3>{}); break;
            default: go(std::integral_constant<int, 4>{}); break;
        }
    }
    if (n_chunks > 0)
        hipLaunchKernelGGL(walk_kernel, dim3(1), dim3(kWalkThreads), 0, st, (const double*)rho, a_dev, K, Kp, T, L, n_chunks,
                           (const double*)starts, (const double*)ends, parallel ? 0 : 1, kForgetTol, (const int*)gate, phi, s,
                           diag_dev);
    if ((rc = g_err.launched("hmmpred filter launch")) != HMMPRED_OK) return rc;

    // 3. closing
    hipLaunchKernelGGL(close_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, (const double*)phi, (const double*)s,
                       (const double*)m, K, Kp, T, lnp_dev, z_dev, end_dev);
    return g_err.launched("hmmpred close_kernel launch");
}

}  // extern "C"
