// include/mtgrow.h: argument checks and the launches of mtgrow_kernels.h.
#include "../../include/mtgrow.h"
#include "../../include/mtree.h"
#include "entry.h"
#include "mtgrow_kernels.h"

namespace mtgrow {
using namespace entry;
ENTRY_SAME_CODES(MTGROW);
static thread_local Err g_err = {""};

static int64_t capacity(int C, int depth) {
    if (C < 2 || C > MTREE_MAX_CHILDREN || depth < 1 || depth > MTREE_MAX_DEPTH) return -1;
    int64_t cap = 0, width = 1;
    for (int d = 0; d <= depth; ++d) {
        cap += width;
        if (cap > MTREE_MAX_NODES) return -1;
        width *= C;
    }
    return cap;
}

// first slot of level d
static int level_lo(int C, int d) {
    int lo = 0, width = 1;
    for (int j = 0; j < d; ++j) {
        lo += width;
        width *= C;
    }
    return lo;
}

static int check_state(const char* who, const mtgrow_state* s, State* out) {
    if (!s) return g_err.fail(MTGROW_EINVAL, "%s: null state", who);
    if (s->n_chains < 1 || s->dim_cont < 0 || s->dim_cat < 0 || s->dim_cont + s->dim_cat < 1 || s->n_post < 1 || s->n < 1)
        return g_err.fail(MTGROW_EINVAL, "%s: n_chains, n and n_post must be >= 1 and there must be a feature", who);
    if (s->n > INT32_MAX) return g_err.fail(MTGROW_EUNSUPPORTED, "%s: more than 2^31 - 1 rows are not supported", who);
    if (s->n_chains > MTREE_MAX_TREES)
        return g_err.fail(MTGROW_EUNSUPPORTED, "%s: more than %d chains are not supported", who, MTREE_MAX_TREES);
    const int64_t cap = capacity(s->n_children, s->max_depth);
    if (cap < 0)
        return g_err.fail(MTGROW_EUNSUPPORTED, "%s: a complete tree of %d children and depth %d has more than %d nodes", who,
                          s->n_children, s->max_depth, MTREE_MAX_NODES);
    if (cap != s->cap) return g_err.fail(MTGROW_EINVAL, "%s: cap is not mtgrow_capacity(n_children, max_depth)", who);
    if (s->threshold != MTGROW_MIDPOINT && s->threshold != MTGROW_KMEANS)
        return g_err.fail(MTGROW_EINVAL, "%s: unknown threshold type", who);
    if (s->dim_cont > 0 && s->xc_dtype != MTREE_F32 && s->xc_dtype != MTREE_F64)
        return g_err.fail(MTGROW_EINVAL, "%s: xc_dtype must be MTREE_F32 or MTREE_F64", who);
    if (s->dim_cat > 0 && (s->xk_dtype < MTREE_U8 || s->xk_dtype > MTREE_I64))
        return g_err.fail(MTGROW_EINVAL, "%s: xk_dtype must be MTREE_U8, MTREE_I32 or MTREE_I64", who);
    if ((s->dim_cont > 0 && !s->xc_dev) || (s->dim_cat > 0 && !s->xk_dev) ||
        (s->dim_cont > 0 && s->threshold == MTGROW_KMEANS && s->n_children == 2 && !s->order_dev))
        return g_err.fail(MTGROW_EINVAL, "%s: null sample pointer", who);
    if (!s->draws_dev || !s->last_feat_dev || !s->last_g_dev || !s->feat_dev || !s->thr_dev || !s->g_dev || !s->post_dev ||
        !s->node_dev || !s->open_dev || !s->regen_dev || !s->dflag_dev || !s->first_dev || !s->count_dev || !s->differs_dev ||
        !s->lo_dev || !s->hi_dev || !s->mid_dev)
        return g_err.fail(MTGROW_EINVAL, "%s: null table", who);
    if (any_misaligned(4, s->order_dev, s->last_feat_dev, s->feat_dev, s->node_dev, s->open_dev, s->regen_dev, s->dflag_dev,
                       s->first_dev, s->count_dev, s->differs_dev) ||
        any_misaligned(8, s->draws_dev, s->last_g_dev, s->thr_dev, s->g_dev, s->post_dev, s->mid_dev) ||
        any_misaligned(8, s->lo_dev, s->hi_dev) ||
        misaligned(s->xc_dev, s->xc_dtype == MTREE_F32 ? 4 : 8) ||
        misaligned(s->xk_dev, s->xk_dtype == MTREE_U8 ? 1 : s->xk_dtype == MTREE_I32 ? 4 : 8))
        return g_err.fail(MTGROW_EINVAL, "%s: misaligned table", who);
    *out = {s->n_chains, s->cap, s->n_children, s->dim_cont, s->dim_cat, s->max_depth, s->n_post, s->threshold, s->n,
            s->xc_dev, s->xk_dev, s->order_dev, s->draws_dev, s->last_feat_dev, s->last_g_dev, s->feat_dev, s->thr_dev,
            s->g_dev, s->post_dev, s->node_dev, s->open_dev, s->regen_dev, s->dflag_dev, s->first_dev, s->count_dev,
            s->differs_dev, (unsigned long long*)s->lo_dev, (unsigned long long*)s->hi_dev, s->mid_dev};
    return MTGROW_OK;
}

#define MTGROW_DISPATCH(xc_dtype, xk_dtype, CALL)                                   \
    do {                                                                           \
        const bool f32_ = (xc_dtype) == MTREE_F32;                                 \
        const int k_ = (xk_dtype) == MTREE_I32 ? 1 : (xk_dtype) == MTREE_I64 ? 2 : 0; \
        if (f32_ && k_ == 0) CALL(float, uint8_t);                                 \
        else if (f32_ && k_ == 1) CALL(float, int32_t);                            \
        else if (f32_) CALL(float, int64_t);                                       \
        else if (k_ == 0) CALL(double, uint8_t);                                   \
        else if (k_ == 1) CALL(double, int32_t);                                   \
        else CALL(double, int64_t);                                                \
    } while (0)
}  // namespace mtgrow

using namespace mtgrow;

extern "C" {

int mtgrow_abi_version(void) { return MTGROW_ABI_VERSION; }
const char* mtgrow_last_error(void) { return g_err.msg; }
int64_t mtgrow_capacity(int n_children, int max_depth) { return capacity(n_children, max_depth); }

int mtgrow_begin(const mtgrow_state* s, double g_root, double g_below, const double* sub_hn_dev, void* stream) {
    State st;
    if (int rc = check_state("mtgrow_begin", s, &st)) return rc;
    if (!sub_hn_dev || misaligned(sub_hn_dev, 8)) return g_err.fail(MTGROW_EINVAL, "mtgrow_begin: null or misaligned sub_hn_dev");
    if (!(g_root >= 0.0 && g_root <= 1.0 && g_below >= 0.0 && g_below <= 1.0))
        return g_err.fail(MTGROW_EINVAL, "mtgrow_begin: g_root and g_below must lie in [0, 1]");
    const int64_t items = (int64_t)st.B * (st.n > st.cap ? st.n : (int64_t)st.cap);
    begin_kernel<<<grid_of(items, kThreads), kThreads, 0, (hipStream_t)stream>>>(st, g_root, g_below,
                                                                                 level_lo(st.C, st.max_depth), sub_hn_dev);
    return g_err.launched("mtgrow_begin");
}

int mtgrow_level(const mtgrow_state* s, int level, int all_regen, double g_max, void* stream) {
    State st;
    if (int rc = check_state("mtgrow_level", s, &st)) return rc;
    if (level < 0 || level >= st.max_depth) return g_err.fail(MTGROW_EINVAL, "mtgrow_level: level must be 0 .. max_depth - 1");
    if (!(g_max >= 0.0 && g_max <= 1.0)) return g_err.fail(MTGROW_EINVAL, "mtgrow_level: g_max must lie in [0, 1]");
    const hipStream_t q = (hipStream_t)stream;
    const int lo = level_lo(st.C, level), hi = level_lo(st.C, level + 1), width = hi - lo;
    const dim3 nodes(grid_of(width, kThreads), st.B), rows(grid_of(st.n, kThreads), st.B);
    decide_kernel<<<nodes, kThreads, 0, q>>>(st, lo, width, all_regen, g_max);
    first_kernel<<<rows, kThreads, 0, q>>>(st, lo, hi);
#define PROBE(TC, TK) probe_kernel<TC, TK><<<rows, kThreads, 0, q>>>(st, lo, hi)
    MTGROW_DISPATCH(s->xc_dtype, s->xk_dtype, PROBE);
#undef PROBE
    if (st.threshold == MTGROW_KMEANS && st.C == 2 && st.dim_cont > 0) {
        const dim3 per_node(width, st.B);
        if (s->xc_dtype == MTREE_F32) kmeans_kernel<float><<<per_node, kKm, 0, q>>>(st, lo);
        else kmeans_kernel<double><<<per_node, kKm, 0, q>>>(st, lo);
    }
    split_kernel<<<nodes, kThreads, 0, q>>>(st, lo, width);
#define ADVANCE(TC, TK) advance_kernel<TC, TK><<<rows, kThreads, 0, q>>>(st, lo, hi)
    MTGROW_DISPATCH(s->xc_dtype, s->xk_dtype, ADVANCE);
#undef ADVANCE
    return g_err.launched("mtgrow_level");
}

int mtgrow_accept(const mtgrow_state* s, int tempered, double g_max, const double* l_new_dev, double* l_last_dev,
                  const double* beta_dev, const double* u_dev, const double* lml_dev, const double* lcm_dev,
                  int32_t* last_feat_dev, double* last_thr_dev, double* last_g_dev, double* last_post_dev,
                  double* last_lml_dev, double* last_lcm_dev, double* out_dev, void* stream) {
    State st;
    if (int rc = check_state("mtgrow_accept", s, &st)) return rc;
    if (!l_new_dev || !l_last_dev || !beta_dev || !u_dev || !lml_dev || !lcm_dev || !last_feat_dev || !last_thr_dev ||
        !last_g_dev || !last_post_dev || !last_lml_dev || !last_lcm_dev || !out_dev)
        return g_err.fail(MTGROW_EINVAL, "mtgrow_accept: null pointer");
    if (any_misaligned(8, l_new_dev, l_last_dev, beta_dev, u_dev, lml_dev, lcm_dev, last_thr_dev, last_g_dev, last_post_dev,
                       last_lml_dev, last_lcm_dev, out_dev) ||
        misaligned(last_feat_dev, 4))
        return g_err.fail(MTGROW_EINVAL, "mtgrow_accept: misaligned pointer");
    if (!(g_max >= 0.0 && g_max <= 1.0)) return g_err.fail(MTGROW_EINVAL, "mtgrow_accept: g_max must lie in [0, 1]");
    accept_kernel<<<st.B, kThreads, 0, (hipStream_t)stream>>>(st, tempered, g_max, l_new_dev, l_last_dev, beta_dev, u_dev,
                                                              lml_dev, lcm_dev, last_feat_dev, last_thr_dev, last_g_dev,
                                                              last_post_dev, last_lml_dev, last_lcm_dev, out_dev);
    return g_err.launched("mtgrow_accept");
}

}  // extern "C"
