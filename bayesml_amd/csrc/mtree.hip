// include/mtree.h: argument checks, the layout of the scratch, and the launches of mtree_kernels.h.
#include "../../include/mtree.h"
#include "entry.h"
#include "mtree_kernels.h"
#include "mtree_lr_kernels.h"

namespace mtree {
using namespace entry;
ENTRY_SAME_CODES(MTREE);
static thread_local Err g_err = {""};

// rows of one call: what grid_of() can hold in a grid's x dimension
constexpr int64_t kMaxRows = (int64_t)0x7fffffff * kThreads;

struct Cols {
    int ni, nr, np;
};

static int cols_of(int family, int degree, Cols* c) {
    if (family < MTREE_BERNOULLI || family > MTREE_LINREG) return MTREE_EINVAL;
    if (family == MTREE_CATEGORICAL || family == MTREE_LINREG) {
        if (degree < 1) return MTREE_EINVAL;
        if (degree > (family == MTREE_LINREG ? MTREE_LR_MAX_DEGREE : MTREE_MAX_DEGREE)) return MTREE_EUNSUPPORTED;
    }
    switch (family) {
        case MTREE_LINREG: *c = {1, lr_tri(degree) + degree + 1, degree + lr_tri(degree) + 3}; break;
        case MTREE_BERNOULLI: *c = {2, 0, 2}; break;
        case MTREE_CATEGORICAL: *c = {1 + degree, 0, degree}; break;
        case MTREE_POISSON: *c = {2, 1, 3}; break;
        case MTREE_EXPONENTIAL: *c = {1, 1, 2}; break;
        default: *c = {1, 3, 5}; break;
    }
    return MTREE_OK;
}

static int check_family(const char* who, int family, int degree, Cols* c) {
    const int rc = cols_of(family, degree, c);
    if (rc == MTREE_EINVAL) return g_err.fail(rc, "%s: unknown family, or degree < 1", who);
    if (rc == MTREE_EUNSUPPORTED && family == MTREE_LINREG)
        return g_err.fail(rc, "%s: a linear-regression degree above %d is not supported (x and y share one 16-column tile)",
                          who, MTREE_LR_MAX_DEGREE);
    if (rc == MTREE_EUNSUPPORTED)
        return g_err.fail(rc, "%s: a categorical degree above %d is not supported", who, MTREE_MAX_DEGREE);
    return MTREE_OK;
}

static int check_forest(const char* who, const mtree_forest* f, Forest* out) {
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

static int check_x(const char* who, const Forest& f, int xc_dtype, const void* xc, int xk_dtype, const void* xk, int64_t n) {
    const char* bad = nullptr;
    if (n < 1) bad = "n must be >= 1";
    else if (n > kMaxRows) bad = "n is too large (more than 2^31 - 1 workgroups of rows)";
    else if (f.dim_cont > 0 && xc_dtype != MTREE_F32 && xc_dtype != MTREE_F64) bad = "xc_dtype must be MTREE_F32 or MTREE_F64";
    else if (f.dim_cat > 0 && (xk_dtype < MTREE_U8 || xk_dtype > MTREE_I64)) bad = "xk_dtype must be MTREE_U8, MTREE_I32 or MTREE_I64";
    else if ((f.dim_cont > 0 && !xc) || (f.dim_cat > 0 && !xk)) bad = "null sample pointer";
    else if (f.dim_cont > 0 && misaligned(xc, xc_dtype == MTREE_F32 ? 4 : 8)) bad = "xc_dev must be aligned to its element size";
    else if (f.dim_cat > 0 && misaligned(xk, xk_dtype == MTREE_U8 ? 1 : xk_dtype == MTREE_I32 ? 4 : 8))
        bad = "xk_dev must be aligned to its element size";
    return bad ? g_err.fail(MTREE_EINVAL, "%s: %s", who, bad) : MTREE_OK;
}

// The six (continuous, categorical) element types.  A dimension of 0 takes the first type of its kind; it is never read.
#define MTREE_DISPATCH(xc_dtype, xk_dtype, CALL)                                   \
    do {                                                                          \
        const bool f32_ = (xc_dtype) == MTREE_F32;                                \
        const int k_ = (xk_dtype) == MTREE_I32 ? 1 : (xk_dtype) == MTREE_I64 ? 2 : 0; \
        if (f32_ && k_ == 0) CALL(float, uint8_t);                                \
        else if (f32_ && k_ == 1) CALL(float, int32_t);                           \
        else if (f32_) CALL(float, int64_t);                                      \
        else if (k_ == 0) CALL(double, uint8_t);                                  \
        else if (k_ == 1) CALL(double, int32_t);                                  \
        else CALL(double, int64_t);                                               \
    } while (0)

// The scratch of mtree_reduce_x in 8-byte slots: offsets of its parts, their sum, and the blocks of the longest tree.
struct LrWork {
    int64_t hist, start, tree_cnt, sorted, slot_key, slot_val, total, nblk;
};
static bool lr_work(int32_t n_nodes, int32_t n_trees, int degree, int64_t n, int n_slabs, LrWork* w) {
    if (n_nodes < 1 || n_trees < 1 || n_trees > n_nodes || degree < 1 || degree > MTREE_LR_MAX_DEGREE || n < 1 ||
        n > INT32_MAX || n_slabs < 1 || n_slabs > MTREE_MAX_SLABS)
        return false;
    const int64_t nr = lr_tri(degree) + degree + 1;
    w->nblk = (n + MTREE_LR_BLOCK - 1) / MTREE_LR_BLOCK;
    w->hist = 0;
    w->start = w->hist + ((int64_t)n_slabs * n_nodes + 1) / 2;
    w->tree_cnt = w->start + ((int64_t)n_nodes + 1) / 2;
    w->sorted = w->tree_cnt + ((int64_t)n_trees + 1) / 2;
    w->slot_key = w->sorted + ((int64_t)n_trees * n + 1) / 2;
    w->slot_val = w->slot_key + (int64_t)n_trees * w->nblk;
    w->total = w->slot_val + (int64_t)n_trees * w->nblk * 2 * nr;
    return true;
}

static bool lds_path(const mtree_forest* f, int cols) { return (int64_t)f->max_tree_nodes * cols <= MTREE_LDS_SLOTS; }
}  // namespace mtree

using namespace mtree;

extern "C" {

int mtree_abi_version(void) { return MTREE_ABI_VERSION; }
const char* mtree_last_error(void) { return g_err.msg; }

int mtree_stat_cols(int family, int degree, int* n_int, int* n_real, int* n_post) {
    Cols c;
    if (int rc = check_family("mtree_stat_cols", family, degree, &c)) return rc;
    if (n_int) *n_int = c.ni;
    if (n_real) *n_real = c.nr;
    if (n_post) *n_post = c.np;
    return MTREE_OK;
}

int64_t mtree_work_len(int32_t n_nodes, int family, int degree, int n_slabs) {
    Cols c;
    if (cols_of(family, degree, &c) != MTREE_OK || n_nodes < 1 || n_slabs < 1 || n_slabs > MTREE_MAX_SLABS) return -1;
    // [ L of the sweep | integer slabs | real slabs ]; normal's second pass (two real columns) takes the place of both
    return (int64_t)n_nodes * (1 + (int64_t)n_slabs * (c.ni + (c.nr > 1 ? 1 : c.nr)));
}

int mtree_route(const mtree_forest* f, int xc_dtype, const void* xc_dev, int xk_dtype, const void* xk_dev,
                const int32_t* cat_card_dev, int64_t n, int32_t* stop_dev, int32_t* path_dev, int64_t* bad_dev, void* stream) {
    Forest F;
    if (int rc = check_forest("mtree_route", f, &F)) return rc;
    if (int rc = check_x("mtree_route", F, xc_dtype, xc_dev, xk_dtype, xk_dev, n)) return rc;
    if (!stop_dev || !bad_dev || (F.dim_cat > 0 && !cat_card_dev)) return g_err.fail(MTREE_EINVAL, "mtree_route: null pointer");
    if (any_misaligned(4, stop_dev, path_dev, cat_card_dev) || misaligned(bad_dev, 8))
        return g_err.fail(MTREE_EINVAL, "mtree_route: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(bad_dev, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return g_err.hip(MTREE_EHIP, "mtree_route: hipMemsetAsync", e);
    const dim3 grid(grid_of(n, kThreads), (unsigned)F.n_trees);
#define MTREE_ROUTE(TC, TK)                                                                                              \
    hipLaunchKernelGGL((route_kernel<TC, TK>), grid, dim3(kThreads), 0, st, F, (const TC*)xc_dev, (const TK*)xk_dev, \
                       cat_card_dev, n, stop_dev, path_dev, (unsigned long long*)bad_dev)
    MTREE_DISPATCH(xc_dtype, xk_dtype, MTREE_ROUTE);
#undef MTREE_ROUTE
    return g_err.launched("route_kernel launch");
}

int mtree_reduce(const mtree_forest* f, int family, int degree, const int32_t* stop_dev, const void* y_dev, int64_t n,
                 int n_slabs, int64_t* stat_int_dev, double* stat_real_dev, void* work_dev, void* stream) {
    Forest F;
    Cols c;
    if (int rc = check_forest("mtree_reduce", f, &F)) return rc;
    if (int rc = check_family("mtree_reduce", family, degree, &c)) return rc;
    if (family == MTREE_LINREG)
        return g_err.fail(MTREE_EINVAL, "mtree_reduce: linear regression needs x: use mtree_reduce_x");
    if (n < 1 || n > kMaxRows) return g_err.fail(MTREE_EINVAL, "mtree_reduce: n must be >= 1 (and at most (2^31 - 1) * 256)");
    if (n_slabs < 1 || n_slabs > MTREE_MAX_SLABS)
        return g_err.fail(MTREE_EINVAL, "mtree_reduce: n_slabs must be in 1..MTREE_MAX_SLABS");
    if (!stop_dev || !y_dev || !stat_int_dev || !work_dev || (c.nr > 0 && !stat_real_dev))
        return g_err.fail(MTREE_EINVAL, "mtree_reduce: null pointer");
    if (misaligned(stop_dev, 4) || any_misaligned(8, y_dev, stat_int_dev, stat_real_dev, work_dev))
        return g_err.fail(MTREE_EINVAL, "mtree_reduce: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const int S = n_slabs, nr1 = c.nr > 1 ? 1 : c.nr;
    unsigned long long* wi = (unsigned long long*)work_dev + F.n_nodes;
    double* wr = (double*)(wi + (int64_t)S * F.n_nodes * c.ni);
    const dim3 grid((unsigned)S, (unsigned)F.n_trees);
    const bool lds1 = lds_path(f, c.ni + nr1);
    if (lds1) {
        hipLaunchKernelGGL((reduce_kernel<true>), grid, dim3(kWave), sizeof(double) * (size_t)f->max_tree_nodes * (c.ni + nr1), st,
                           F, family, degree, c.ni, nr1, stop_dev, y_dev, (const double*)nullptr, n, S, wi, wr);
    } else {
        const hipError_t e = hipMemsetAsync(wi, 0, sizeof(double) * (size_t)S * F.n_nodes * (c.ni + nr1), st);
        if (e != hipSuccess) return g_err.hip(MTREE_EHIP, "mtree_reduce: hipMemsetAsync", e);
        hipLaunchKernelGGL((reduce_kernel<false>), grid, dim3(kWave), 0, st, F, family, degree, c.ni, nr1, stop_dev, y_dev,
                           (const double*)nullptr, n, S, wi, wr);
    }
    if (int rc = g_err.launched("reduce_kernel launch")) return rc;
    hipLaunchKernelGGL((combine_kernel<int64_t>), dim3(grid_of((int64_t)F.n_nodes * c.ni, kThreads)), dim3(kThreads), 0, st,
                       (const int64_t*)wi, S, (int64_t)F.n_nodes, c.ni, c.ni, 0, stat_int_dev);
    if (int rc = g_err.launched("combine_kernel launch")) return rc;
    if (nr1 > 0) {
        hipLaunchKernelGGL((combine_kernel<double>), dim3(grid_of(F.n_nodes, kThreads)), dim3(kThreads), 0, st,
                           (const double*)wr, S, (int64_t)F.n_nodes, 1, c.nr, 0, stat_real_dev);
        if (int rc = g_err.launched("combine_kernel launch")) return rc;
    }
    if (family != MTREE_NORMAL) return MTREE_OK;
    // The second pass: two columns per node, in the scratch of the first pass (ni + 1 = 2 columns, combined already).
    static_assert(sizeof(unsigned long long) == sizeof(double), "the two passes share the slabs");
    double* w2 = (double*)wi;
    if (lds_path(f, 2)) {
        hipLaunchKernelGGL((reduce_centred_kernel<true>), grid, dim3(kWave), sizeof(double) * (size_t)f->max_tree_nodes * 2, st, F,
                           stop_dev, (const double*)y_dev, n, S, (const int64_t*)stat_int_dev, (const double*)stat_real_dev, c.nr,
                           w2);
    } else {
        const hipError_t e = hipMemsetAsync(w2, 0, sizeof(double) * (size_t)S * F.n_nodes * 2, st);
        if (e != hipSuccess) return g_err.hip(MTREE_EHIP, "mtree_reduce: hipMemsetAsync", e);
        hipLaunchKernelGGL((reduce_centred_kernel<false>), grid, dim3(kWave), 0, st, F, stop_dev, (const double*)y_dev, n, S,
                           (const int64_t*)stat_int_dev, (const double*)stat_real_dev, c.nr, w2);
    }
    if (int rc = g_err.launched("reduce_centred_kernel launch")) return rc;
    hipLaunchKernelGGL((combine_kernel<double>), dim3(grid_of((int64_t)F.n_nodes * 2, kThreads)), dim3(kThreads), 0, st,
                       (const double*)w2, S, (int64_t)F.n_nodes, 2, c.nr, 1, stat_real_dev);
    return g_err.launched("combine_kernel launch");
}

int64_t mtree_reduce_x_work_len(int32_t n_nodes, int32_t n_trees, int degree, int64_t n, int n_slabs) {
    LrWork w;
    return lr_work(n_nodes, n_trees, degree, n, n_slabs, &w) ? w.total : -1;
}

int mtree_reduce_x(const mtree_forest* f, int family, int degree, const int32_t* stop_dev, int x_dtype, const void* x_dev,
                   int64_t x_stride, const double* y_dev, int64_t n, int n_slabs, int64_t* stat_int_dev,
                   double* stat_real_dev, void* work_dev, void* stream) {
    Forest F;
    Cols c;
    if (int rc = check_forest("mtree_reduce_x", f, &F)) return rc;
    if (int rc = check_family("mtree_reduce_x", family, degree, &c)) return rc;
    if (family != MTREE_LINREG)
        return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: only linear regression reduces x: use mtree_reduce");
    if (n < 1 || n > INT32_MAX) return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: n must be in 1..2^31 - 1");
    if (n_slabs < 1 || n_slabs > MTREE_MAX_SLABS)
        return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: n_slabs must be in 1..MTREE_MAX_SLABS");
    if (x_dtype != MTREE_F32 && x_dtype != MTREE_F64)
        return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: x_dtype must be MTREE_F32 or MTREE_F64");
    if (x_stride < degree) return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: x_stride must be >= degree");
    if (!stop_dev || !x_dev || !y_dev || !stat_int_dev || !stat_real_dev || !work_dev)
        return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: null pointer");
    if (misaligned(stop_dev, 4) || misaligned(x_dev, x_dtype == MTREE_F32 ? 4 : 8) ||
        any_misaligned(8, y_dev, stat_int_dev, stat_real_dev, work_dev))
        return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: misaligned pointer");
    LrWork w;
    if (!lr_work(F.n_nodes, F.n_trees, degree, n, n_slabs, &w))
        return g_err.fail(MTREE_EINVAL, "mtree_reduce_x: inconsistent sizes");
    hipStream_t st = (hipStream_t)stream;
    int64_t* base = (int64_t*)work_dev;
    int32_t* hist = (int32_t*)(base + w.hist);
    int32_t* start = (int32_t*)(base + w.start);
    int32_t* tree_cnt = (int32_t*)(base + w.tree_cnt);
    int32_t* sorted = (int32_t*)(base + w.sorted);
    int32_t* slot_key = (int32_t*)(base + w.slot_key);
    double* slot_val = (double*)(base + w.slot_val);
    // a node without rows keeps zeros: only the nodes of the sorted array are written below
    const hipError_t e = hipMemsetAsync(stat_real_dev, 0, sizeof(double) * (size_t)F.n_nodes * c.nr, st);
    if (e != hipSuccess) return g_err.hip(MTREE_EHIP, "mtree_reduce_x: hipMemsetAsync", e);
    const dim3 slabs((unsigned)n_slabs, (unsigned)F.n_trees);
    hipLaunchKernelGGL(lr_hist_kernel, slabs, dim3(kThreads), 0, st, F, stop_dev, n, n_slabs, hist);
    if (int rc = g_err.launched("lr_hist_kernel launch")) return rc;
    hipLaunchKernelGGL(lr_scan_kernel, dim3((unsigned)F.n_trees), dim3(kThreads), 0, st, F, n_slabs, c.ni, hist, start,
                       stat_int_dev, tree_cnt);
    if (int rc = g_err.launched("lr_scan_kernel launch")) return rc;
    hipLaunchKernelGGL(lr_scatter_kernel, slabs, dim3(kWave), 0, st, F, stop_dev, n, n_slabs, (const int32_t*)hist, sorted);
    if (int rc = g_err.launched("lr_scatter_kernel launch")) return rc;
    const dim3 blocks((unsigned)w.nblk, (unsigned)F.n_trees);
    if (x_dtype == MTREE_F32)
        hipLaunchKernelGGL((lr_gram_kernel<float>), blocks, dim3(kWave), 0, st, F, degree, (const float*)x_dev, x_stride, y_dev,
                           n, (const int32_t*)sorted, (const int32_t*)start, (const int64_t*)stat_int_dev, c.ni,
                           (const int32_t*)tree_cnt, c.nr, stat_real_dev, slot_key, slot_val);
    else
        hipLaunchKernelGGL((lr_gram_kernel<double>), blocks, dim3(kWave), 0, st, F, degree, (const double*)x_dev, x_stride,
                           y_dev, n, (const int32_t*)sorted, (const int32_t*)start, (const int64_t*)stat_int_dev, c.ni,
                           (const int32_t*)tree_cnt, c.nr, stat_real_dev, slot_key, slot_val);
    if (int rc = g_err.launched("lr_gram_kernel launch")) return rc;
    hipLaunchKernelGGL(lr_fixup_kernel, dim3((unsigned)(2 * w.nblk), (unsigned)F.n_trees), dim3(kWave), 0, st, F.n_nodes, c.nr,
                       (const int32_t*)slot_key, (const double*)slot_val, stat_real_dev);
    return g_err.launched("lr_fixup_kernel launch");
}

int64_t mtree_values_len(int32_t n_nodes, int family, int degree) {
    Cols c;
    if (cols_of(family, degree, &c) != MTREE_OK || n_nodes < 1) return -1;
    if (family == MTREE_LINREG) return (int64_t)n_nodes * (degree + lr_tri(degree) + 2);
    return (int64_t)n_nodes * (degree > 2 ? degree : 2);
}

int mtree_sweep(const mtree_forest* f, int family, int degree, int64_t* stat_int_dev, double* stat_real_dev,
                const double* h0_dev, double* post_dev, double* g_dev, double* lml_dev, double* lcm_dev, double* lnp_dev,
                void* work_dev, void* stream) {
    Forest F;
    Cols c;
    if (int rc = check_forest("mtree_sweep", f, &F)) return rc;
    if (int rc = check_family("mtree_sweep", family, degree, &c)) return rc;
    if (!stat_int_dev || (c.nr > 0 && !stat_real_dev) || !h0_dev || !post_dev || !g_dev || !lml_dev || !lcm_dev || !lnp_dev ||
        !work_dev)
        return g_err.fail(MTREE_EINVAL, "mtree_sweep: null pointer");
    if (any_misaligned(8, stat_int_dev, stat_real_dev, h0_dev, post_dev, g_dev, lml_dev, lcm_dev, lnp_dev, work_dev))
        return g_err.fail(MTREE_EINVAL, "mtree_sweep: misaligned pointer");
    if (family == MTREE_LINREG) {
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(lr_prior_kernel, dim3(1), dim3(1), 0, st, degree, h0_dev, (double*)work_dev + F.n_nodes);
        if (int rc = g_err.launched("lr_prior_kernel launch")) return rc;
        hipLaunchKernelGGL(lr_sweep_kernel, dim3((unsigned)F.n_trees), dim3(kThreads), 0, st, F, degree, c.ni, c.nr, c.np,
                           stat_int_dev, stat_real_dev, h0_dev, post_dev, g_dev, lml_dev, lcm_dev, lnp_dev, (double*)work_dev);
        return g_err.launched("lr_sweep_kernel launch");
    }
    hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)F.n_trees), dim3(kThreads), 0, (hipStream_t)stream, F, family, degree, c.ni,
                       c.nr, c.np, stat_int_dev, stat_real_dev, h0_dev, post_dev, g_dev, lml_dev, lcm_dev, lnp_dev,
                       (double*)work_dev);
    return g_err.launched("sweep_kernel launch");
}

int mtree_predict(const mtree_forest* f, int family, int degree, int mode, int xc_dtype, const void* xc_dev, int xk_dtype,
                  const void* xk_dev, int64_t n, const double* post_dev, const double* g_dev, const double* prob_dev,
                  double* values_dev, void* out_dev, void* stream) {
    Forest F;
    Cols c;
    if (int rc = check_forest("mtree_predict", f, &F)) return rc;
    if (int rc = check_family("mtree_predict", family, degree, &c)) return rc;
    if (mode < MTREE_PRED_MEAN || mode > MTREE_PRED_VAR) return g_err.fail(MTREE_EINVAL, "mtree_predict: unknown mode");
    const bool clf = family == MTREE_BERNOULLI || family == MTREE_CATEGORICAL;
    if ((mode == MTREE_PRED_MEAN && clf) || ((mode == MTREE_PRED_PROBA || mode == MTREE_PRED_CLASS) && !clf) ||
        (mode == MTREE_PRED_VAR && family != MTREE_NORMAL && family != MTREE_LINREG))
        return g_err.fail(MTREE_EINVAL, "mtree_predict: the family has no such read-out");
    if (family == MTREE_LINREG && degree != F.dim_cont)
        return g_err.fail(MTREE_EINVAL, "mtree_predict: the linear-regression degree must equal dim_cont");
    if (int rc = check_x("mtree_predict", F, xc_dtype, xc_dev, xk_dtype, xk_dev, n)) return rc;
    if (!post_dev || !g_dev || !prob_dev || !values_dev || !out_dev) return g_err.fail(MTREE_EINVAL, "mtree_predict: null pointer");
    if (any_misaligned(8, post_dev, g_dev, prob_dev, values_dev, out_dev))
        return g_err.fail(MTREE_EINVAL, "mtree_predict: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (family == MTREE_LINREG) {
        hipLaunchKernelGGL(lr_values_kernel, dim3(grid_of(F.n_nodes, kThreads)), dim3(kThreads), 0, st, F.n_nodes, degree, c.np,
                           post_dev, values_dev);
        if (int rc = g_err.launched("lr_values_kernel launch")) return rc;
#define MTREE_LR_PREDICT(TC, TK)                                                                                     \
    hipLaunchKernelGGL((lr_predict_kernel<TC, TK>), dim3(grid_of(n, kThreads)), dim3(kThreads), 0, st, F, mode, degree, \
                       (const TC*)xc_dev, (const TK*)xk_dev, n, g_dev, prob_dev, (const double*)values_dev, (double*)out_dev)
        MTREE_DISPATCH(xc_dtype, xk_dtype, MTREE_LR_PREDICT);
#undef MTREE_LR_PREDICT
        return g_err.launched("lr_predict_kernel launch");
    }
    const int C = family == MTREE_BERNOULLI ? 2 : family == MTREE_CATEGORICAL ? degree : 1;
    hipLaunchKernelGGL(values_kernel, dim3(grid_of(F.n_nodes, kThreads)), dim3(kThreads), 0, st, F.n_nodes, family, degree, mode,
                       c.np, C, post_dev, values_dev);
    if (int rc = g_err.launched("values_kernel launch")) return rc;
#define MTREE_PREDICT(TC, TK)                                                                                   \
    hipLaunchKernelGGL((predict_kernel<TC, TK>), dim3(grid_of(n, kThreads)), dim3(kThreads), 0, st, F, mode, C, \
                       (const TC*)xc_dev, (const TK*)xk_dev, n, g_dev, prob_dev, (const double*)values_dev, out_dev)
    MTREE_DISPATCH(xc_dtype, xk_dtype, MTREE_PREDICT);
#undef MTREE_PREDICT
    return g_err.launched("predict_kernel launch");
}

}  // extern "C"
