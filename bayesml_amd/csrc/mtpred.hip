// include/mtpred.h: argument checks, the choice between the staged and the direct form, and the launches of
// mtpred_kernels.h.
#include "../../include/mtpred.h"

#include "entry.h"
#include "mtpred_kernels.h"

namespace mtpred {
using namespace entry;
ENTRY_SAME_CODES(MTREE);
static thread_local Err g_err = {""};

// rows of one call: a tile per workgroup in the grid's x dimension
constexpr int64_t kMaxRows = (int64_t)0x7fffffff * kTile;

// (doubles of a node's constants, length of its posterior vector), or a status code
static int family_cols(int family, int degree, int* CL, int* np) {
    if (family < MTREE_BERNOULLI || family > MTREE_LINREG) return MTREE_EINVAL;
    if (family == MTREE_CATEGORICAL || family == MTREE_LINREG) {
        if (degree < 1) return MTREE_EINVAL;
        if (degree > (family == MTREE_LINREG ? MTREE_LR_MAX_DEGREE : MTREE_MAX_DEGREE)) return MTREE_EUNSUPPORTED;
    }
    const int tri = degree * (degree + 1) / 2;
    switch (family) {
        case MTREE_BERNOULLI: *CL = 2, *np = 2; break;
        case MTREE_CATEGORICAL: *CL = degree, *np = degree; break;
        case MTREE_POISSON: *CL = 3, *np = 3; break;
        case MTREE_EXPONENTIAL: *CL = 3, *np = 2; break;
        case MTREE_NORMAL: *CL = 4, *np = 5; break;
        default: *CL = kLrConsts, *np = degree + tri + 3; break;
    }
    return MTREE_OK;
}

static int check_forest(const mtree_forest* f, Forest* out) {
    const char* who = "mtpred_logpdf";
    if (!f) return g_err.fail(MTREE_EINVAL, "%s: null forest", who);
    if (f->n_trees < 1 || f->n_nodes < f->n_trees || f->n_thr < 0 || f->max_tree_nodes < 1 || f->max_children < 0 ||
        f->max_depth < 0 || f->dim_cont < 0 || f->dim_cat < 0 || f->dim_cont + f->dim_cat < 1 ||
        f->max_tree_nodes > f->n_nodes)
        return g_err.fail(MTREE_EINVAL, "%s: inconsistent forest sizes", who);
    if (f->n_trees > MTREE_MAX_TREES || f->max_tree_nodes > MTREE_MAX_NODES || f->max_children > MTREE_MAX_CHILDREN ||
        f->max_depth > MTREE_MAX_DEPTH)
        return g_err.fail(MTREE_EUNSUPPORTED,
                          "%s: more than %d trees, %d nodes per tree, %d children per node or depth %d is not supported", who,
                          MTREE_MAX_TREES, MTREE_MAX_NODES, MTREE_MAX_CHILDREN, MTREE_MAX_DEPTH);
    if (!f->tree_off_dev || !f->feat_dev || !f->child0_dev || !f->nchild_dev || !f->thr_off_dev || !f->depth_dev ||
        (f->n_thr > 0 && !f->thr_dev))
        return g_err.fail(MTREE_EINVAL, "%s: null forest table", who);
    if (any_misaligned(4, f->tree_off_dev, f->feat_dev, f->child0_dev, f->nchild_dev, f->thr_off_dev, f->depth_dev) ||
        misaligned(f->thr_dev, 8))
        return g_err.fail(MTREE_EINVAL, "%s: misaligned forest table", who);
    *out = {f->n_trees, f->n_nodes, f->n_thr, f->max_depth, f->dim_cont, f->dim_cat, f->tree_off_dev, f->feat_dev,
            f->child0_dev, f->nchild_dev, f->thr_off_dev, f->depth_dev, f->thr_dev};
    return MTREE_OK;
}

static_assert(MTPRED_SHARE >= 1 && MTPRED_SHARE <= kTile + 1, "1 = always the matrix pipe, kTile + 1 = never");
}  // namespace mtpred

using namespace mtpred;

extern "C" {

int mtpred_abi_version(void) { return MTPRED_ABI_VERSION; }
const char* mtpred_last_error(void) { return g_err.msg; }

int64_t mtpred_consts_len(int32_t n_nodes, int family, int degree) {
    int CL, np;
    if (family_cols(family, degree, &CL, &np) != MTREE_OK || n_nodes < 1) return -1;
    return (int64_t)n_nodes * CL;
}

int64_t mtpred_work_len(int64_t n, int total) {
    if (n < 1 || n > kMaxRows) return -1;
    return total ? (n + kTile - 1) / kTile : 0;
}

int mtpred_logpdf(const mtree_forest* forest, int family, int degree, int xc_dtype, const void* xc_dev, int xk_dtype,
                  const void* xk_dev, const void* y_dev, int64_t n, const double* post_dev, const double* g_dev,
                  const double* prob_dev, double* consts_dev, double* lnp_dev, double* total_dev, void* work_dev,
                  void* stream) {
    Forest F;
    int CL, np;
    if (int rc = check_forest(forest, &F)) return rc;
    const int rc = family_cols(family, degree, &CL, &np);
    if (rc == MTREE_EINVAL) return g_err.fail(rc, "mtpred_logpdf: unknown family, or degree < 1");
    if (rc == MTREE_EUNSUPPORTED)
        return g_err.fail(rc, "mtpred_logpdf: a degree above %d (categorical) or %d (linear regression) is not supported",
                          MTREE_MAX_DEGREE, MTREE_LR_MAX_DEGREE);
    if (family == MTREE_LINREG && degree != F.dim_cont)
        return g_err.fail(MTREE_EINVAL, "mtpred_logpdf: the linear-regression degree must equal dim_cont");
    const char* bad = nullptr;
    if (n < 1) bad = "n must be >= 1";
    else if (n > kMaxRows) bad = "n is too large (more than 2^31 - 1 tiles of rows)";
    else if (F.dim_cont > 0 && xc_dtype != MTREE_F32 && xc_dtype != MTREE_F64) bad = "xc_dtype must be MTREE_F32 or MTREE_F64";
    else if (F.dim_cat > 0 && (xk_dtype < MTREE_U8 || xk_dtype > MTREE_I64)) bad = "xk_dtype must be MTREE_U8, MTREE_I32 or MTREE_I64";
    else if ((F.dim_cont > 0 && !xc_dev) || (F.dim_cat > 0 && !xk_dev) || !y_dev || !post_dev || !g_dev || !prob_dev ||
             !consts_dev || !lnp_dev || (total_dev && !work_dev))
        bad = "null pointer";
    else if (F.dim_cont > 0 && misaligned(xc_dev, xc_dtype == MTREE_F32 ? 4 : 8)) bad = "xc_dev must be aligned to its element size";
    else if (F.dim_cat > 0 && misaligned(xk_dev, xk_dtype == MTREE_U8 ? 1 : xk_dtype == MTREE_I32 ? 4 : 8))
        bad = "xk_dev must be aligned to its element size";
    else if (any_misaligned(8, y_dev, post_dev, g_dev, prob_dev, consts_dev, lnp_dev, total_dev, work_dev))
        bad = "y_dev and the tables must be 8-byte aligned";
    if (bad) return g_err.fail(MTREE_EINVAL, "mtpred_logpdf: %s", bad);

    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(consts_kernel, dim3(grid_of(F.n_nodes, 256)), dim3(256), 0, st, F.n_nodes, family, degree, np, CL,
                       post_dev, consts_dev);
    if (int e = g_err.launched("consts_kernel launch")) return e;
    const int64_t tiles = (n + kTile - 1) / kTile;
    const size_t stage = (size_t)kTile * (sizeof(double) * F.dim_cont + sizeof(int32_t) * F.dim_cat);
    const bool staged = stage <= (size_t)kLdsBytes;
    double* tile_sum = total_dev ? (double*)work_dev : nullptr;
#define MTPRED_PASS(FAM, STAGED)                                                                                          \
    hipLaunchKernelGGL((pass_kernel<FAM, STAGED>), dim3((unsigned)tiles), dim3(kThreads), (STAGED) ? stage : 0, st, F, degree, \
                       np, CL, xc_dtype, xc_dev, xk_dtype, xk_dev, (const long long*)y_dev, n, post_dev, g_dev, prob_dev,  \
                       (const double*)consts_dev, MTPRED_SHARE, lnp_dev, tile_sum)
#define MTPRED_FAMILY(FAM)         \
    case FAM:                      \
        if (staged) MTPRED_PASS(FAM, true); \
        else MTPRED_PASS(FAM, false);       \
        break
    switch (family) {
        MTPRED_FAMILY(MTREE_BERNOULLI);
        MTPRED_FAMILY(MTREE_CATEGORICAL);
        MTPRED_FAMILY(MTREE_POISSON);
        MTPRED_FAMILY(MTREE_EXPONENTIAL);
        MTPRED_FAMILY(MTREE_NORMAL);
        MTPRED_FAMILY(MTREE_LINREG);
    }
#undef MTPRED_FAMILY
#undef MTPRED_PASS
    if (int e = g_err.launched("pass_kernel launch")) return e;
    if (total_dev) {
        hipLaunchKernelGGL(total_kernel, dim3(1), dim3(256), 0, st, (const double*)tile_sum, tiles, total_dev);
        return g_err.launched("total_kernel launch");
    }
    return MTREE_OK;
}

}  // extern "C"
