// C ABI of the GMM-VB data-pass engine, the M-step: gmmvb_load_responsibilities, gmmvb_mstep, gmmvb_estep_mstep (include/gmmvb.h; shared helpers in capi_internal.h).
#include "capi_internal.h"
#include "mstep_plan.h"

extern "C" {

int gmmvb_load_responsibilities(gmmvb_workspace* ws, const double* r_dev, int64_t n_rows, void* stream) {
    if (!ws || !r_dev) return fail(GMMVB_EINVAL, "null argument");
    if (n_rows < 1 || n_rows > ws->max_rows) return fail(GMMVB_EINVAL, "n_rows must be in [1, max_rows]");
    claim_scratch(ws);
    const int tb = 256;
    hipLaunchKernelGGL(load_r_kernel, dim3((unsigned)((n_rows + tb - 1) / tb)), dim3(tb), 0, (hipStream_t)stream,
                       r_dev, n_rows, ws->K, ws->lnrho, ws->npad, ws->lse, ws->sorted ? ws->iperm : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GMMVB_EHIP, "load_r launch", e);
    ws->e_state = 2;
    ws->lost_estep = false;
    ws->e_rows = n_rows;
    ws->n_spans = 0;
    ws->bounds_rows = 0;               // the array holds responsibilities now, nothing a later E-step may carry over
    drop_settled_rows(ws);
    ws->rec_valid = false;
    ws->dense_valid = false;
    ws->rec_live = false;
    ws->act_rows = 0;
    return GMMVB_OK;
}

}  // extern "C"

namespace {

// One M-step in flight: the call's arguments, what the plan (mstep_plan.h) said, and the kernel the info line names.
struct Mstep {
    gmmvb_workspace* ws;
    const void* x_dev;
    int64_t ldx, n_rows;
    double* stats_dev;
    hipStream_t st;
    bool vec;
    MstepPlan plan{};
    const char* name = "";
    int runs = 0;          // list form: the runs of its last launch (launch_mstep_list), 0 = chunks

    MstepFacts facts() const;
    void begin_phase() const {
        if (phase_events(ws)) note_hip(ws, hipEventRecord(ws->ev[2], st));
    }
    int prologue();
    template <typename X>
    void launch_generic(const double* lr, const double* aux) const;
    int run_generic();
    int reduce_and_note();
    int apply_delta(const MstepListArgs& la, int nblk);
    int build_lists(int nblk);
    int run_lists();
    int run_dense();
};

// What the pass needs before its form matters - and the plan's refusal, once the steps the M-step takes before it finds out
// are done (the list form's own refusal comes behind its delta lists: run_lists).
int Mstep::prologue() {
    if (plan.need_row_lse) {         // a mixture M-step on an HMM workspace: the log-normaliser after all
        hipLaunchKernelGGL(row_lse_kernel, dim3((unsigned)((n_rows + kLseRows - 1) / kLseRows)), dim3(256), 0, st, ws->lnrho,
                           ws->npad, n_rows, ws->K, ws->lse, nullptr, nullptr, 1);
        ws->lse_stale = false;
    }
    if (plan.need_prepare) {
        // (multivariate_normal.LearnModel's one-pass moments call gmmvb_mstep straight after gmmvb_load_responsibilities)
        const int rc = gmmvb_prepare_rows(ws, x_dev, ldx, n_rows, st);
        if (rc) return rc;
    }
    if (plan.need_gamma_cm && hmm_ensure_gamma_cm(ws->hmm, st) != hipSuccess) return fail(GMMVB_EHIP, "gamma transpose launch");
    if (plan.status != GMMVB_OK && plan.kind != kMstepLists) return fail(plan.status, plan.message);
    return GMMVB_OK;
}

template <typename X>
void Mstep::launch_generic(const double* lr, const double* aux) const {
    const int S = (int)plan.S;
    hipLaunchKernelGGL(mstep_generic_first_kernel<X>, dim3(ws->K, S), dim3(256), 0, st, (const X*)x_dev, ldx, n_rows, ws->D,
                       ws->pivot, lr, ws->lse, aux, ws->npad, ws->K, plan.rows_per_split, plan.direct_r, ws->gen_first);
    hipLaunchKernelGGL(mstep_generic_second_kernel<X>, dim3(tri_pairs(ws->T), ws->K, S), dim3(256), 0, st, (const X*)x_dev, ldx,
                       n_rows, ws->D, ws->pivot, lr, ws->lse, aux, ws->npad, ws->K, plan.rows_per_split, plan.direct_r, ws->T,
                       ws->gen_second);
}

// c_degree > 256 (generic.h): plain f64 kernels on the caller's rows, per row split (a failed launch is reported behind the
// reduce kernel)
int Mstep::run_generic() {
    const double* lr = plan.gamma_weights ? hmm_gamma_cm(ws->hmm) : ws->lnrho;
    const double* aux = plan.aux_lnrho ? ws->lnrho : nullptr;
    begin_phase();
    span_begin(ws, kSpanMstepMain, st);
    if (ws->x_dtype == GMMVB_F64)
        launch_generic<double>(lr, aux);
    else
        launch_generic<float>(lr, aux);
    span_end(ws, st);
    ++ws->passes[plan.counter];
    return GMMVB_OK;
}

// The tail of every form: the end of the profile's M phase, the slabs (or chunks, with the cache of settled rows) summed
// into the caller's statistics block, and the M-step's segment of the info line.
int Mstep::reduce_and_note() {
    if (phase_events(ws)) {
        note_hip(ws, hipEventRecord(ws->ev[3], st));
        ws->ev_m = true;
    }
    const bool generic = plan.reduce == kReduceGeneric;
    const int tiles = tri_pairs(ws->T);
    span_begin(ws, kSpanReduce, st);
    if (generic) {
        const int64_t elems = ws->D + 2 + (int64_t)tiles * 256;
        hipLaunchKernelGGL(reduce_generic_kernel, dim3((unsigned)((elems + 255) / 256), ws->K), dim3(256), 0, st, ws->gen_first,
                           ws->gen_second, (int)plan.S, ws->K, ws->D, ws->T, stats_dev);
    } else if (plan.reduce == kReduceChunks) {
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3((plan.elems + 255) / 256, ws->K), dim3(256), 0, st, ws->slabs, ws->plan_m,
                           ws->K, ws->D, ws->T, stats_dev, 0, plan.add_cache ? ws->cache : nullptr, ws->counts, runs);
    } else {
        hipLaunchKernelGGL(reduce_stats_kernel, dim3((plan.elems + 255) / 256, ws->K), dim3(256), 0, st, ws->slabs, (int)plan.S,
                           ws->K, ws->D, ws->T, stats_dev);
    }
    span_end(ws, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GMMVB_EHIP, generic ? "mstep_generic launch" : "reduce_stats launch", e);
    const size_t used = std::strlen(ws->info);
    if (generic)
        std::snprintf(ws->info + used, sizeof(ws->info) - used, " | mstep_generic_f64<D=%d> tiles=%d splits=%d", ws->D, tiles,
                      (int)plan.S);
    else
        std::snprintf(ws->info + used, sizeof(ws->info) - used, " | %s grid=%lldx%d splits=%lld rows/split=%lld", name,
                      (long long)plan.grid, mstep_threads(ws->T, plan.pre), (long long)plan.S, (long long)plan.rows_per_split);
    return take_hip(ws, "event record inside the M-step");
}

// The rows that settled or came loose in this pass enter / leave the cache of settled rows: signed lists from
// rec_finish_kernel's delta masks, the list kernel over them, and their sums added to the cache.
int Mstep::apply_delta(const MstepListArgs& la, int nblk) {
    span_begin(ws, kSpanLists, st);
    // (qpart: the delta and M-step pairs rec_finish_kernel counted per block - none of either: nothing to fill)
    scan_and_fill(ws, st, ws->dmask, ws->dblk, nblk, n_rows, ws->K, plan.qpart ? ws->qpart : nullptr, ws->lock, ws->lcomp);
    span_end(ws, st);
    MstepListArgs ld = la;
    ld.direct_r = 3;
    const char* dname = "";
    span_begin(ws, kSpanMstepMain, st);
    const hipError_t e = launch_mstep_list(ws->T, (int)plan.dgrid, st, ld, &dname, &runs);
    span_end(ws, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "settled-row delta launch", e);
    span_begin(ws, kSpanReduce, st);
    hipLaunchKernelGGL(reduce_chunks_kernel, dim3((plan.elems + 255) / 256, ws->K), dim3(256), 0, st, ws->slabs, ws->plan_m, ws->K,
                       ws->D, ws->T, ws->cache, 1, nullptr, ws->counts, runs);
    span_end(ws, st);
    return GMMVB_OK;
}

// The pass's own lists: from the M-step's masks (the rows in the cache left out) or from the E-step's full ones.
int Mstep::build_lists(int nblk) {
    span_begin(ws, kSpanLists, st);
    if (plan.build == kBuildMmask)
        scan_and_fill(ws, st, ws->mmask, ws->mblk, nblk, n_rows, ws->K, plan.qpart ? ws->qpart : nullptr);
    else
        scan_and_fill(ws, st, ws->masks, ws->blk, nblk, n_rows, ws->K);
    const hipError_t e = hipGetLastError();
    span_end(ws, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "active-sample lists", e);
    return GMMVB_OK;
}

// E-step output: only the samples that can change the f64 sums, through per-component lists (the list building is part of
// the M-step's time)
int Mstep::run_lists() {
    const int nblk = (int)((n_rows + kSelRows - 1) / kSelRows);
    begin_phase();
    MstepListArgs la{ws->xc, ws->lnrho, ws->lse, ws->lists, ws->npad, ws->counts, ws->plan_m, plan.cap_chunks, plan.r_min,
                     ws->npad, ws->K, ws->slabs};
    la.num_cu = ws->num_cu, la.runs_cap = ws->opt_mlist_runs;
    if (plan.rows != kRowsCentred) {
        la.x32 = (const float*)(plan.rows == kRowsXp32 ? ws->xp : x_dev);
        la.ldx = plan.list_ldx;
        la.n_rows = n_rows;
        la.D = ws->D;
        la.pivot = ws->pivot;
    }
    if (plan.need_recenter) {        // this list kernel reads the centred copy: bring it to the internal row order
        const hipError_t e = recenter_rows(ws, n_rows, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "center_rows launch", e);
    }
    if (plan.apply_delta) {
        const int rc = apply_delta(la, nblk);
        if (rc) return rc;
        ws->delta_pending = ws->active_lists = ws->mlists_done = false;      // (whatever becomes of the call from here on)
    }
    if (plan.status != GMMVB_OK) return fail(plan.status, plan.message);
    if (plan.build != kBuildNone) {
        const int rc = build_lists(nblk);
        if (rc) return rc;
    }
    ws->delta_pending = plan.delta_pending;
    ws->mlists_done = plan.mlists_done;
    ws->active_lists = plan.active_lists;
    if (plan.clear_blk_fresh) ws->blk_fresh = false;
    span_begin(ws, kSpanMstepMain, st);
    const hipError_t e = launch_mstep_list(ws->T, (int)plan.grid, st, la, &name, &runs);
    span_end(ws, st);
    ++ws->passes[plan.counter];
    if (e != hipSuccess) return fail(GMMVB_EHIP, "mstep launch", e);
    return GMMVB_OK;
}

// every pair of (row, component): the MFMA kernels over the centred copy or the caller's rows, the one-tile kernels, the
// wide kernel (launch_mstep goes there past 8 feature tiles)
int Mstep::run_dense() {
    ++ws->passes[plan.counter];
    begin_phase();
    if (plan.need_recenter) {        // the dense kernel reads the centred copy: bring it to the internal row order
        const hipError_t e = recenter_rows(ws, n_rows, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "center_rows launch", e);
    }
    const int Dp = 16 * ws->T;
    const MstepArgs a{plan.pre ? ws->xc : x_dev, plan.pre ? Dp : ldx, n_rows, plan.pre ? Dp : ws->D, ws->pivot,
                      plan.gamma_weights ? hmm_gamma_cm(ws->hmm) : ws->lnrho, ws->lse, plan.aux_lnrho ? ws->lnrho : nullptr,
                      ws->npad, ws->K, plan.KG, (int)plan.S, plan.rows_per_split, plan.direct_r, ws->slabs};
    hipError_t e;
    span_begin(ws, kSpanMstepMain, st);
    if (plan.kind == kMstepHmmSmall) {
        e = launch_hmm_mstep_small((int)plan.grid, st, a, plan.KGW, hmm_gamma_tm(ws->hmm), hmm_padded_states(ws->hmm),
                                   plan.hmm_sparse_walk, &name);
    } else if (plan.kind == kMstepSmall) {
        e = launch_mstep_small((int)plan.grid, st, a, plan.KGW, kMstepSmallCw, &name);
    } else {
        const double pairs = (double)n_rows * ws->K;
        const bool cal = plan.may_calibrate && cal_wanted(ws, 1, pairs);
        if (cal) note_hip(ws, hipEventRecord(ws->cal_ev[2], st));
        e = launch_mstep(ws->T, ws->x_dtype == GMMVB_F64, vec, plan.pre, (int)plan.grid, st, a, &name);
        if (cal) cal_mark(ws, 1, pairs, st);
    }
    span_end(ws, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "mstep launch", e);
    return GMMVB_OK;
}

// What plan_mstep reads (mstep_plan.h), from the workspace and this call's matrix.
MstepFacts Mstep::facts() const {
    MstepFacts f;
    f.e_state = ws->e_state, f.e_rows = ws->e_rows, f.n_rows = n_rows, f.ldx = ldx;
    f.K = ws->K, f.D = ws->D, f.T = ws->T, f.x_dtype = ws->x_dtype;
    f.vec = vec;
    f.generic = ws->generic, f.wide = ws->wide;
    f.has_xc = ws->xc != nullptr, f.xc_of_x = xc_is_of(ws, x_dev, ldx, n_rows), f.xc_stale = ws->xc_stale;
    f.sorted = ws->sorted, f.has_xp = ws->xp != nullptr;
    f.sparse = ws->sparse, f.has_masks = ws->masks != nullptr, f.act_rows = ws->act_rows;
    f.rec_live = ws->rec_live, f.lock_live = ws->lock_live, f.delta_pending = ws->delta_pending;
    f.mlists_done = ws->mlists_done, f.mlists_lost = ws->mlists_lost, f.active_lists = ws->active_lists;
    f.S_cap = ws->S_cap, f.split_rows = ws->split_rows, f.gen_S = ws->gen_S;
    if (!ws->generic) f.kpw_pre = mstep_components_per_wg(ws->T, true), f.kpw_raw = mstep_components_per_wg(ws->T, false);
    f.lse_stale = ws->lse_stale, f.hmm_no_lnrho = ws->hmm_no_lnrho, f.hmm_skip_h = ws->hmm_skip_h;
    f.opt_hmm_mstep_dense = ws->opt_hmm_mstep_dense, f.opt_mlist_xc = ws->opt_mlist_xc;
    f.lag_valid = ws->lag.valid, f.lag_act = ws->lag.act, f.list_m_below = ws->pt.list_m_below();
    return f;
}

}  // namespace

extern "C" {

int gmmvb_mstep(gmmvb_workspace* ws, const void* x_dev, int64_t ldx, int64_t n_rows, double* stats_dev,
                void* stream) {
    bool vec = false;
    int rc = check_x(ws, x_dev, ldx, n_rows, &vec);
    if (rc) return rc;
    if (!stats_dev) return fail(GMMVB_EINVAL, "stats_dev is null");
    Mstep m{ws, x_dev, ldx, n_rows, stats_dev, (hipStream_t)stream, vec};
    MstepFacts facts = m.facts();
    if (mstep_needs_counters(facts)) {
        // after a dense E-step the host has been waiting for that kernel anyway: read this pass's own count
        rc = fetch_counters(ws);
        if (rc) return rc;
        facts.lag_valid = ws->lag.valid, facts.lag_act = ws->lag.act;
    }
    m.plan = plan_mstep(facts);
    rc = m.prologue();
    if (rc) return rc;
    rc = m.plan.kind == kMstepGeneric ? m.run_generic() : (m.plan.kind == kMstepLists ? m.run_lists() : m.run_dense());
    return rc ? rc : m.reduce_and_note();
}

int gmmvb_estep_mstep(gmmvb_workspace* ws, const void* x_dev, int64_t ldx, int64_t n_rows, double* stats_dev,
                      void* stream) {
    int rc = gmmvb_estep(ws, x_dev, ldx, n_rows, stream);
    if (rc) return rc;
    return gmmvb_mstep(ws, x_dev, ldx, n_rows, stats_dev, stream);
}

}  // extern "C"
