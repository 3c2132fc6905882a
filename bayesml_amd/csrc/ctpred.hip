// include/ctpred.h: argument checks and the piece plan in plain C++, and the launches of ctpred_kernels.h.
#include "../../include/ctpred.h"
#include "../../include/ctsp.h"
#include "ctpred_kernels.h"
#include "ctree_shape.h"

namespace ctpred {
using namespace entry;
ENTRY_SAME_CODES(CTPRED);
static_assert(CTPRED_TILE == kThreads && CTPRED_PIECE == kPiece, "ctpred.h and ctpred_kernels.h disagree");
static thread_local Err g_err = {""};

static int group_width(int k) {
    int W = 1;
    while (W < k && W < 64) W *= 2;
    return W;
}

static int elem_size(int d) { return d == CTPRED_U8 ? 1 : d == CTPRED_I32 ? 4 : 8; }

// The levels of a (k, D) tree on dense tables; b = 0.
static int dense_levels(const char* who, int k, int D, Levels* lv) {
    ctree_shape::Shape sh;
    const int rc = ctree_shape::shape_of(k, D, &sh);
    if (rc == CTPRED_EINVAL) return g_err.fail(rc, "%s: k and D must be >= 1", who);
    if (rc == CTPRED_EUNSUPPORTED)
        return g_err.fail(rc, "%s: k > %d or k^(D+1) > %d is not supported", who, CTREE_MAX_K, CTREE_MAX_SLOTS);
    for (int d = 0; d <= D + 1; ++d) lv->off[d] = sh.off[d];
    for (int d = D + 2; d <= kMaxLevels; ++d) lv->off[d] = sh.off[D + 1];
    return CTPRED_OK;
}

// The levels of ctsp.h's tables from the caller's `off`, and b = bits per symbol.
static int sparse_levels(const char* who, int k, int D, const int64_t* off, Levels* lv, int* b) {
    if (k < 1 || D < 1) return g_err.fail(CTPRED_EINVAL, "%s: k and D must be >= 1", who);
    *b = 1;
    while ((1 << *b) < k) ++*b;
    if (k > CTSP_MAX_K || (int64_t)*b * D > CTSP_MAX_KEY_BITS)
        return g_err.fail(CTPRED_EUNSUPPORTED, "%s: k > %d or ceil(log2 k) * D > %d is not supported", who, CTSP_MAX_K,
                          CTSP_MAX_KEY_BITS);
    if (!off) return g_err.fail(CTPRED_EINVAL, "%s: null pointer", who);
    if (off[0] != 0) return g_err.fail(CTPRED_EINVAL, "%s: off[0] must be 0", who);
    for (int d = 0; d <= D; ++d) {
        const int64_t cap = off[d + 1] - off[d];
        if (cap < 2 || (cap & (cap - 1)) != 0 || cap > ((int64_t)1 << 30))
            return g_err.fail(CTPRED_EINVAL, "%s: the capacity of level %d must be a power of two in 2..2^30", who, d);
    }
    for (int d = 0; d <= D + 1; ++d) lv->off[d] = off[d];
    for (int d = D + 2; d <= kMaxLevels; ++d) lv->off[d] = off[D + 1];
    return CTPRED_OK;
}

static int launch_rowsum(const char* who, int k, int D, int has_tree, const Levels& lv, const void* key_dev, const void* beta_dev,
                         const void* exists_dev, const void* hn_beta_dev, void* rowsum_dev, void* stream) {
    if (!hn_beta_dev || !rowsum_dev || (has_tree && (!beta_dev || !exists_dev)))
        return g_err.fail(CTPRED_EINVAL, "%s: null pointer", who);
    if (any_misaligned(8, key_dev, beta_dev, hn_beta_dev, rowsum_dev)) return g_err.fail(CTPRED_EINVAL, "%s: misaligned pointer", who);
    const int W = group_width(k);
    const int64_t slots = lv.off[D + 1], rows = has_tree ? slots + 1 : 1;
    int64_t grid = (rows + kThreads / W - 1) / (kThreads / W);
    if (grid > kMaxGrid) grid = kMaxGrid;
    hipLaunchKernelGGL(rowsum_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, (const u64*)key_dev,
                       (const uint8_t*)exists_dev, (const double*)beta_dev, slots, has_tree, k, W, (const double*)hn_beta_dev,
                       (double*)rowsum_dev);
    return g_err.launched("ctpred rowsum_kernel launch");
}

struct PassArgs {
    int dtype;
    const void* x;
    int64_t n;
    const void* seq_off;
    int64_t S;
    int k, b, D, has_tree;
    Levels lv;
    Tables t;
    double hn_g;
    const void* hn_beta;
    void *lnp, *argmax, *rows, *status;
    hipStream_t st;
};

template <bool SPARSE, bool STACK, typename T>
static int launch_one(const PassArgs& a, int W, int count_bad, double* lnp, int64_t* argmax, double* rows) {
    const int per = kThreads / W;
    const size_t lds = (size_t)((per + a.D + 3) & ~3) + (STACK ? (size_t)a.D * kThreads * sizeof(int32_t) : 0);
    hipLaunchKernelGGL((pass_kernel<SPARSE, STACK, T>), dim3(grid_of(a.n, per)), dim3(kThreads), lds, a.st, (const T*)a.x, a.n,
                       (const int64_t*)a.seq_off, a.S, a.k, a.b, a.D, a.has_tree, a.lv, a.t, a.hn_g, (const double*)a.hn_beta, W,
                       count_bad, lnp, argmax, rows, (u64*)a.status);
    return g_err.launched("ctpred pass_kernel launch");
}

// The scalar launch when lnp is asked for, the vector launch when argmax or rows are; the first of them counts the symbols.
template <bool SPARSE, bool STACK, typename T>
static int launch_both(const PassArgs& a) {
    int first = 1;
    if (a.lnp) {
        if (int rc = launch_one<SPARSE, STACK, T>(a, 1, first, (double*)a.lnp, nullptr, nullptr)) return rc;
        first = 0;
    }
    if (a.argmax || a.rows) return launch_one<SPARSE, STACK, T>(a, group_width(a.k), first, nullptr, (int64_t*)a.argmax, (double*)a.rows);
    return CTPRED_OK;
}

template <bool SPARSE, bool STACK>
static int launch_dtype(const PassArgs& a) {
    if (a.dtype == CTPRED_U8) return launch_both<SPARSE, STACK, uint8_t>(a);
    if (a.dtype == CTPRED_I32) return launch_both<SPARSE, STACK, int32_t>(a);
    return launch_both<SPARSE, STACK, int64_t>(a);
}

// What both passes check once the levels are known.
static int check_pass(const char* who, const PassArgs& a, bool sparse) {
    if (a.dtype < CTPRED_U8 || a.dtype > CTPRED_I64)
        return g_err.fail(CTPRED_EINVAL, "%s: dtype must be CTPRED_U8, CTPRED_I32 or CTPRED_I64", who);
    if (a.n < 1) return g_err.fail(CTPRED_EINVAL, "%s: n must be >= 1", who);
    if (a.n >= ((int64_t)1 << 31)) return g_err.fail(CTPRED_EUNSUPPORTED, "%s: n must be below 2^31", who);
    if (a.S < 0 || a.S > a.n + ((int64_t)1 << 31) || (a.S > 0) != (a.seq_off != nullptr))
        return g_err.fail(CTPRED_EINVAL, "%s: seq_off_dev and S >= 1 go together", who);
    if (!a.x || !a.t.rowsum || !a.hn_beta || !a.status) return g_err.fail(CTPRED_EINVAL, "%s: null pointer", who);
    if (a.has_tree && (!a.t.beta || !a.t.g || !a.t.exists || (sparse && !a.t.key)))
        return g_err.fail(CTPRED_EINVAL, "%s: null pointer", who);
    if (!a.lnp && !a.argmax && !a.rows) return g_err.fail(CTPRED_EINVAL, "%s: no output asked for", who);
    if (!(a.hn_g >= 0.0 && a.hn_g <= 1.0)) return g_err.fail(CTPRED_EINVAL, "%s: hn_g must be in [0, 1]", who);
    if (misaligned(a.x, elem_size(a.dtype))) return g_err.fail(CTPRED_EINVAL, "%s: x_dev must be aligned to its element size", who);
    if (any_misaligned(8, a.seq_off, (const void*)a.t.key, (const void*)a.t.beta, (const void*)a.t.g, (const void*)a.t.rowsum, a.hn_beta,
                       (const void*)a.lnp, (const void*)a.argmax, (const void*)a.rows, (const void*)a.status))
        return g_err.fail(CTPRED_EINVAL, "%s: misaligned pointer", who);
    const hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int64_t) * CTPRED_STATUS_LEN, a.st);
    if (e != hipSuccess) return g_err.hip(CTPRED_EHIP, "ctpred: hipMemsetAsync", e);
    return CTPRED_OK;
}
}  // namespace ctpred

using namespace ctpred;

extern "C" {

int ctpred_abi_version(void) { return CTPRED_ABI_VERSION; }
const char* ctpred_last_error(void) { return g_err.msg; }

int ctpred_group_width(int k) { return k < 1 || k > 256 ? -1 : group_width(k); }

int ctpred_rowsum_dense(int k, int D, int has_tree, const void* beta_dev, const void* exists_dev, const void* hn_beta_dev,
                        void* rowsum_dev, void* stream) {
    Levels lv;
    if (int rc = dense_levels("ctpred_rowsum_dense", k, D, &lv)) return rc;
    return launch_rowsum("ctpred_rowsum_dense", k, D, has_tree, lv, nullptr, beta_dev, exists_dev, hn_beta_dev, rowsum_dev, stream);
}

int ctpred_rowsum_sparse(int k, int D, int has_tree, const int64_t* off, const void* key_dev, const void* beta_dev,
                         const void* exists_dev, const void* hn_beta_dev, void* rowsum_dev, void* stream) {
    Levels lv;
    int b;
    if (int rc = sparse_levels("ctpred_rowsum_sparse", k, D, off, &lv, &b)) return rc;
    if (has_tree && !key_dev) return g_err.fail(CTPRED_EINVAL, "ctpred_rowsum_sparse: null pointer");
    return launch_rowsum("ctpred_rowsum_sparse", k, D, has_tree, lv, has_tree ? key_dev : nullptr, beta_dev, exists_dev,
                         hn_beta_dev, rowsum_dev, stream);
}

int ctpred_pass_dense(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, int64_t S, int k, int D, int has_tree,
                      const void* beta_dev, const void* g_dev, const void* exists_dev, const void* rowsum_dev, double hn_g,
                      const void* hn_beta_dev, void* lnp_dev, void* argmax_dev, void* rows_dev, void* status_dev, void* stream) {
    PassArgs a = {dtype, x_dev, n, seq_off_dev, S, k, 0, D, has_tree, {}, {}, hn_g, hn_beta_dev, lnp_dev, argmax_dev, rows_dev,
                  status_dev, (hipStream_t)stream};
    if (int rc = dense_levels("ctpred_pass_dense", k, D, &a.lv)) return rc;
    a.t = Tables{nullptr, (const double*)beta_dev, (const double*)g_dev, (const uint8_t*)exists_dev, (const double*)rowsum_dev};
    if (int rc = check_pass("ctpred_pass_dense", a, false)) return rc;
    return launch_dtype<false, false>(a);
}

int ctpred_pass_sparse(int dtype, const void* x_dev, int64_t n, const void* seq_off_dev, int64_t S, int k, int D, int has_tree,
                       const int64_t* off, const void* key_dev, const void* beta_dev, const void* g_dev,
                       const void* exists_dev, const void* rowsum_dev, double hn_g, const void* hn_beta_dev, int upwalk,
                       void* lnp_dev, void* argmax_dev, void* rows_dev, void* status_dev, void* stream) {
    PassArgs a = {dtype, x_dev, n, seq_off_dev, S, k, 0, D, has_tree, {}, {}, hn_g, hn_beta_dev, lnp_dev, argmax_dev, rows_dev,
                  status_dev, (hipStream_t)stream};
    if (int rc = sparse_levels("ctpred_pass_sparse", k, D, off, &a.lv, &a.b)) return rc;
    if (upwalk != CTPRED_UP_STACK && upwalk != CTPRED_UP_PROBE)
        return g_err.fail(CTPRED_EINVAL, "ctpred_pass_sparse: upwalk must be CTPRED_UP_STACK or CTPRED_UP_PROBE");
    a.t = Tables{(const u64*)key_dev, (const double*)beta_dev, (const double*)g_dev, (const uint8_t*)exists_dev,
                 (const double*)rowsum_dev};
    if (int rc = check_pass("ctpred_pass_sparse", a, true)) return rc;
    return upwalk == CTPRED_UP_STACK ? launch_dtype<true, true>(a) : launch_dtype<true, false>(a);
}

int64_t ctpred_plan_pieces(const int64_t* seq_off, int64_t S, int64_t* piece_off) {
    if (!seq_off || S < 1 || seq_off[0] != 0) return -1;
    int64_t at = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t len = seq_off[s + 1] - seq_off[s];
        if (len < 0) return -1;
        if (piece_off) piece_off[s] = at;
        at += (len + kPiece - 1) / kPiece;
    }
    if (piece_off) piece_off[S] = at;
    return at;
}

int ctpred_totals(const void* lnp_dev, int64_t n, const void* seq_off_dev, const void* piece_off_dev, int64_t S,
                  int64_t pieces, void* partial_dev, void* totals_dev, void* stream) {
    if (n < 0 || S < 1 || pieces < 0) return g_err.fail(CTPRED_EINVAL, "ctpred_totals: n and pieces must be >= 0 and S >= 1");
    if (pieces > n || pieces >= ((int64_t)1 << 31) || S >= ((int64_t)1 << 32))
        return g_err.fail(CTPRED_EINVAL, "ctpred_totals: more pieces than positions, or more sequences than 2^32");
    if (!totals_dev || !seq_off_dev || (pieces > 0 && (!lnp_dev || !piece_off_dev || !partial_dev)))
        return g_err.fail(CTPRED_EINVAL, "ctpred_totals: null pointer");
    if (any_misaligned(8, lnp_dev, seq_off_dev, piece_off_dev, (const void*)partial_dev, (const void*)totals_dev))
        return g_err.fail(CTPRED_EINVAL, "ctpred_totals: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (pieces > 0) {
        hipLaunchKernelGGL(piece_sum_kernel, dim3((unsigned)pieces), dim3(kThreads), 0, st, (const double*)lnp_dev, n,
                           (const int64_t*)seq_off_dev, (const int64_t*)piece_off_dev, S, (double*)partial_dev);
        if (int rc = g_err.launched("ctpred piece_sum_kernel launch")) return rc;
    }
    hipLaunchKernelGGL(seq_sum_kernel, dim3(grid_of(S, kThreads / 64)), dim3(kThreads), 0, st, (const double*)partial_dev,
                       pieces > 0 ? (const int64_t*)piece_off_dev : nullptr, S, pieces, (double*)totals_dev);
    return g_err.launched("ctpred seq_sum_kernel launch");
}

}  // extern "C"
