// include/hmmbatch.h: the argument checks and the launches of hmmbatch_kernels.h behind hmmpred's per-row stage.
//
// hmm.h defines its non-template kernels with external linkage, and hmm_capi.o and hmmpred.o already hold them: this object
// compiles the header under a namespace of its own, as hmmpred.hip does.
#define gmmvb gmmvb_hmmbatch
#include "../../include/hmmbatch.h"
#include "../../include/hmmpred.h"
#include "entry.h"
#include "hmmbatch_kernels.h"
#include "hmmpred_emit.h"

#include <type_traits>

namespace hmmbatch {
ENTRY_SAME_CODES(HMMBATCH);
static_assert(HMMBATCH_MAX_DEGREE == HMMPRED_MAX_DEGREE && HMMBATCH_MAX_STATES == HMMPRED_MAX_STATES, "the emission is hmmpred's");
static_assert((int)HMMBATCH_F32 == (int)HMMPRED_F32 && (int)HMMBATCH_F64 == (int)HMMPRED_F64, "the dtype passes through");
ENTRY_SAME_CODES(HMMPRED);      // (and so does emit_rows' status)
static_assert(HMMBATCH_MAX_STATES == kWideThreads, "batch_walk_wide_kernel: a thread per state");
static_assert(HMMBATCH_MFMA_STATES == 64, "hmm.h: KT <= 4 blocks of 16 states");
static_assert(HMMBATCH_SHEAF == kSheaf, "a sheaf is the MFMA's 16 columns");
static thread_local entry::Err g_err = {""};

// The scratch of a call, in doubles from its start.
struct Layout {
    int Kp;
    int64_t npad, rho, m, lne, total;
};
static Layout layout(int K, int64_t n_rows) {
    Layout l;
    l.Kp = 16 * ((K + 15) / 16);
    l.npad = (n_rows + 63) / 64 * 64;
    l.rho = 0;
    l.m = l.rho + l.npad * l.Kp;
    l.lne = l.m + l.npad;
    l.total = l.lne + l.npad * K;
    return l;
}

static const char* check_shape(int K, int D, int64_t n_rows, int64_t n_seq) {
    if (K < 1) return "K must be >= 1";
    if (D < 1 || D > HMMBATCH_MAX_DEGREE) return "D must be in 1..19200";
    if (n_rows < 0) return "n_rows must be >= 0";
    if (n_seq < 1 || n_seq > INT32_MAX) return "n_seq must be in 1..2^31-1";
    return nullptr;
}

static int launch_totals(int64_t n_seq, const int64_t* off, const double* lnp, double* tot, hipStream_t st) {
    hipLaunchKernelGGL(segment_totals_kernel, dim3(entry::grid_of(n_seq, kWavesPerGroup)), dim3(64 * kWavesPerGroup), 0, st, off,
                       lnp, n_seq, tot);
    return g_err.launched("hmmbatch segment_totals_kernel launch");
}
}  // namespace hmmbatch

using namespace hmmbatch;

extern "C" {

int hmmbatch_abi_version(void) { return HMMBATCH_ABI_VERSION; }
const char* hmmbatch_last_error(void) { return g_err.msg; }

int64_t hmmbatch_scratch_len(int K, int D, int64_t n_rows, int64_t n_seq) {
    if (check_shape(K, D, n_rows, n_seq) || K > HMMBATCH_MAX_STATES) return -1;
    return layout(K, n_rows).total;
}

int hmmbatch_logpdf(int K, int D, int x_dtype, const void* x_dev, int64_t ldx, int64_t n_rows, int64_t n_seq,
                    const int64_t* off_dev, const int32_t* order_dev, const double* pivot_dev, const double* img_dev,
                    const double* c_dev, const double* nu_dev, const double* a_dev, const double* w0_dev, int64_t w0_stride,
                    double* scratch_dev, double* lnp_dev, int64_t* z_dev, double* end_dev, double* tot_dev, void* stream) {
    const char* who = "hmmbatch_logpdf";
    if (const char* bad = check_shape(K, D, n_rows, n_seq)) return g_err.fail(HMMBATCH_EINVAL, "%s: %s", who, bad);
    if (K > HMMBATCH_MAX_STATES)
        return g_err.fail(HMMBATCH_EUNSUPPORTED, "%s: at most %d states in this version (got %d)", who, HMMBATCH_MAX_STATES, K);
    if (x_dtype != HMMBATCH_F32 && x_dtype != HMMBATCH_F64)
        return g_err.fail(HMMBATCH_EINVAL, "%s: x_dtype must be HMMBATCH_F32 or HMMBATCH_F64", who);
    if (ldx < D) return g_err.fail(HMMBATCH_EINVAL, "%s: ldx must be >= D", who);
    if (w0_stride != 0 && w0_stride != K) return g_err.fail(HMMBATCH_EINVAL, "%s: w0_stride must be 0 or K", who);
    if (!off_dev || !order_dev || !pivot_dev || !img_dev || !c_dev || !nu_dev || !a_dev || !w0_dev || !end_dev ||
        (n_rows > 0 && (!x_dev || !scratch_dev || !lnp_dev)))
        return g_err.fail(HMMBATCH_EINVAL, "%s: null pointer", who);
    const size_t esz = x_dtype == HMMBATCH_F32 ? 4 : 8;
    if (entry::misaligned(x_dev, esz)) return g_err.fail(HMMBATCH_EINVAL, "%s: x must be aligned to its element size", who);
    if (entry::any_misaligned(8, pivot_dev, c_dev, nu_dev, a_dev, w0_dev, lnp_dev, end_dev, tot_dev) ||
        entry::misaligned(z_dev, 8) || entry::misaligned(off_dev, 8) || entry::misaligned(order_dev, 4))
        return g_err.fail(HMMBATCH_EINVAL, "%s: the double and int64 arrays must be 8-byte aligned, order_dev 4-byte", who);
    if (entry::misaligned(img_dev, 16) || entry::misaligned(scratch_dev, 16))
        return g_err.fail(HMMBATCH_EINVAL, "%s: img_dev and scratch_dev must be 16-byte aligned", who);

    const hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(K, n_rows);
    double* const rho = scratch_dev + l.rho;
    double* const m = scratch_dev + l.m;

    // 1. the rows: ln e, then rho' (lane order) and m - hmmpred's, over the whole batch
    if (n_rows > 0) {
        const int rc = hmmpred::emit_rows(K, D, x_dtype, x_dev, ldx, n_rows, pivot_dev, img_dev, c_dev, nu_dev, scratch_dev + l.lne,
                                          l.npad, rho, m, st);
        if (rc != HMMBATCH_OK) return g_err.fail(rc, "%s: %s", who, hmmpred_last_error());
    }

    // 2. the recursion: sheaves of 16 sequences in `order`, four to a workgroup; a workgroup per sequence above 64 states
    if (K <= HMMBATCH_MFMA_STATES) {
        const unsigned grid = entry::grid_of(n_seq, kSheaf * kWavesPerGroup);
        auto go = [&](auto kt) {
            hipLaunchKernelGGL((batch_walk_mfma_kernel<decltype(kt)::value>), dim3(grid), dim3(64 * kWavesPerGroup), 0, st,
                               (const double*)rho, (const double*)m, a_dev, K, off_dev, order_dev, n_seq, w0_dev, w0_stride, lnp_dev,
                               z_dev, end_dev);
        };
        switch (l.Kp / 16) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 3: go(std::integral_constant<int, 3>{}); break;
            default: go(std::integral_constant<int, 4>{}); break;
        }
    } else {
        hipLaunchKernelGGL(batch_walk_wide_kernel, dim3((unsigned)n_seq), dim3(kWideThreads), 0, st, (const double*)rho,
                           (const double*)m, a_dev, K, l.Kp, off_dev, order_dev, w0_dev, w0_stride, lnp_dev, z_dev, end_dev);
    }
    const int rc = g_err.launched("hmmbatch recursion launch");
    if (rc != HMMBATCH_OK || tot_dev == nullptr) return rc;

    // 3. closing
    return launch_totals(n_seq, off_dev, lnp_dev, tot_dev, st);
}

int hmmbatch_totals(int64_t n_seq, const int64_t* off_dev, const double* lnp_dev, double* tot_dev, void* stream) {
    const char* who = "hmmbatch_totals";
    if (n_seq < 1 || n_seq > INT32_MAX) return g_err.fail(HMMBATCH_EINVAL, "%s: n_seq must be in 1..2^31-1", who);
    if (!off_dev || !tot_dev) return g_err.fail(HMMBATCH_EINVAL, "%s: null pointer", who);   // (lnp may be: no rows at all)
    if (entry::misaligned(off_dev, 8) || entry::any_misaligned(8, lnp_dev, tot_dev))
        return g_err.fail(HMMBATCH_EINVAL, "%s: the double and int64 arrays must be 8-byte aligned", who);
    return launch_totals(n_seq, off_dev, lnp_dev, tot_dev, (hipStream_t)stream);
}

}  // extern "C"
