// C ABI of the GMM-VB data-pass engine, the E-step: gmmvb_estep and the passes it is made of (include/gmmvb.h; shared helpers in capi_internal.h).
#include "capi_internal.h"

namespace {

// One E-step in flight: what its launches share, what the plan (pass_plan.h) said, and what the pass did - for finish().
struct Pass {
    gmmvb_workspace* ws;
    const void* x_dev;
    int64_t ldx, n_rows;
    hipStream_t st;
    int is64;
    bool vec;
    int sel_grid;
    double pairs;
    EstepArgs a{};
    EstepI8Args a8{};
    RecArrays rec{};
    bool i8 = false;
    bool prunable = false;           // a pruned pass may follow this one: a counted dense pass builds its records
    bool prev_lists = false, can_project = false, own_known = false, tmeta_was_valid = false;
    bool quiet_was_valid = false;    // the tile state of the settled rows described the arrays when the pass began (workspace.h)
    // the plan
    int mode = kPassDense;
    bool settle = false, proof_capable = false;
    double skip_margin = -1.0;
    // the outcome
    bool counted = false, proof_ran = false, tmeta_kept = false, projected = false, filtered = false, emission_to_hmm = false,
         sorted_now = false;
    bool quiet_swept = false;        // the sweep counted the tiles' loose rows (tile_loose is this pass's)
    bool phase_closed = false;       // the pass recorded the end of the profile's E phase itself
    const char* name = "";           // the info line (nullptr: the pass wrote its own)
    int rpw = 0;
    int64_t grid = 0;

    PassFacts facts();
    int apply(const PassFacts& f, const PassPlan& plan);
    int run_generic();
    int run_dense();
    int run_bound();
    int run_sweep();
    int run_sweep_over_lists();
    int run_sweep_from_best();
    int sweep_bounds(bool proof, bool own_round);
    int run_candidates();
    int finish(const char* latch_what);
};

// Regroup the internal row order by the best component of the last E-step (aux_kernels.h): new permutation, permuted copy
// of x, centred copy rebuilt from it.  Everything row-indexed in the workspace is stale afterwards: the caller (a bound
// pass) rebuilds it.
hipError_t regroup_rows(gmmvb_workspace* ws, const void* x_dev, int64_t ldx, int64_t n_rows, hipStream_t st, bool keep_state,
                        bool margin_ok) {
    const int sel_grid = (int)((n_rows + kSelRows - 1) / kSelRows);
    const unsigned cgrid = (unsigned)((n_rows + 255) / 256);
    const int* key = ws->khat;                  // best components in the order the second pass sorts
    const int* perm_in = ws->sorted ? ws->perm : nullptr;
    // Two stable counting sorts, least significant key first: how firmly the rows sit in their component
    // (margin_bucket_kernel; needs the last pass's log-normalisers), then the component.
    const bool by_margin = ws->opt_regroup_margin && margin_ok && ws->K >= kMarginBuckets;
    if (by_margin) {
        int* bucket = ws->perm_tmp;             // (free until the first composition below writes it)
        hipLaunchKernelGGL(margin_bucket_kernel, dim3(cgrid), dim3(256), 0, st, ws->lnrho, ws->npad, n_rows, ws->lse, ws->khat,
                           keep_state ? ws->lock : nullptr, bucket);
        hipLaunchKernelGGL(select_mask_kernel<3>, dim3(sel_grid), dim3(kSelRows), 0, st, ws->lnrho, ws->npad, n_rows,
                           kMarginBuckets, bucket, ws->masks, ws->blk);
        scan_and_fill(ws, st, ws->masks, ws->blk, sel_grid, n_rows, kMarginBuckets);
        // the best components and the caller's rows in the intermediate order (the keys in the records' slot array, which
        // the bound pass rewrites anyway)
        int* key1 = reinterpret_cast<int*>(ws->rec_d);
        hipLaunchKernelGGL(perm_compose_kernel, dim3(cgrid, kMarginBuckets), dim3(256), 0, st, ws->lists, ws->npad, ws->counts,
                           ws->khat, key1);
        hipLaunchKernelGGL(perm_compose_kernel, dim3(cgrid, kMarginBuckets), dim3(256), 0, st, ws->lists, ws->npad, ws->counts,
                           perm_in, ws->perm_tmp);
        key = key1;
        perm_in = ws->perm_tmp;
    }
    hipLaunchKernelGGL(select_mask_kernel<3>, dim3(sel_grid), dim3(kSelRows), 0, st, ws->lnrho, ws->npad, n_rows, ws->K,
                       const_cast<int*>(key), ws->masks, ws->blk);
    scan_and_fill(ws, st, ws->masks, ws->blk, sel_grid, n_rows, ws->K);
    ws->tile_ref_valid = false;
    if (ws->tile_ref) {                // the groups' lengths are in counts now: every tile's reference component (project.h)
        if (launch_proj_tile_ref(ws->counts, ws->K, sel_grid, ws->tile_ref, st) == hipSuccess) ws->tile_ref_valid = true;
    }
    if (by_margin) {
        // (three row-sized index buffers in rotation: the new order goes where the best components were - the bound pass
        // that follows rewrites them)
        hipLaunchKernelGGL(perm_compose_kernel, dim3(cgrid, ws->K), dim3(256), 0, st, ws->lists, ws->npad, ws->counts, perm_in,
                           ws->khat);
        int* new_perm = ws->khat;
        ws->khat = ws->perm_tmp;
        ws->perm_tmp = ws->perm;
        ws->perm = new_perm;
    } else {
        hipLaunchKernelGGL(perm_compose_kernel, dim3(cgrid, ws->K), dim3(256), 0, st, ws->lists, ws->npad, ws->counts, perm_in,
                           ws->perm_tmp);
        std::swap(ws->perm, ws->perm_tmp);
    }
    if (keep_state) {
        // the cache of single-component rows is a sum over rows - it does not care about their order; what is kept per row
        // (in the cache or not, for which component, the settled rows' distance bound) moves with the rows.  The records'
        // byte arrays and the threshold array are free at this point of a bound pass (rec_build_kernel rewrites them).
        hipLaunchKernelGGL(regroup_state_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, ws->perm,
                           ws->sorted ? ws->iperm : nullptr, n_rows, ws->lock, ws->lcomp, ws->dlock, ws->rec_sel, ws->rec_flags,
                           ws->rthr);
        std::swap(ws->lock, ws->rec_sel);
        std::swap(ws->lcomp, ws->rec_flags);
        std::swap(ws->dlock, ws->rthr);
    }
    hipLaunchKernelGGL(perm_invert_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, ws->perm, n_rows, ws->iperm);
    const int64_t total = n_rows * ws->D;
    const unsigned pg = (unsigned)((total + 255) / 256);
    const int64_t esz = ws->x_dtype == GMMVB_F64 ? 8 : 4;
    if ((ws->D * esz) % 16 == 0 && (ldx * esz) % 16 == 0 && (uintptr_t)x_dev % 16 == 0) {
        const int p16 = (int)(ws->D * esz / 16);
        hipLaunchKernelGGL(permute_rows16_kernel, dim3((unsigned)((n_rows * p16 + 255) / 256)), dim3(256), 0, st,
                           (const uint4*)x_dev, ldx * esz / 16, n_rows, p16, ws->perm, (uint4*)ws->xp);
    } else if (ws->x_dtype == GMMVB_F64)
        hipLaunchKernelGGL(permute_rows_kernel<double>, dim3(pg), dim3(256), 0, st, (const double*)x_dev, ldx, n_rows, ws->D,
                           ws->perm, (double*)ws->xp);
    else
        hipLaunchKernelGGL(permute_rows_kernel<float>, dim3(pg), dim3(256), 0, st, (const float*)x_dev, ldx, n_rows, ws->D,
                           ws->perm, (float*)ws->xp);
    // the centred f64 copy follows the internal order too, but it is only read by the dense M-step (and by the list
    // M-step of f64 / ragged-D inputs): rebuilt there when needed (recenter_rows), not here - 4 ms and 10 GB at C3
    ws->xc_stale = ws->xc != nullptr;
    if (ws->xq && ws->xq_src == x_dev) {       // the digit planes follow the internal order (3 ms at C3, once or twice per fit)
        hipError_t eq = launch_x_digits(ws->xp, ws->x_dtype == GMMVB_F64, ws->D, n_rows, ws->D, ws->pivot, ws->xq, ws->xqe, st);
        if (eq != hipSuccess) return eq;
        ws->xq_gen = ws->pivot_gen;
    }
    ws->sorted = true;
    ++ws->sorts;
    return hipGetLastError();
}

// bound pass of the pruned E-step: an upper bound of ln rho for every pair (three int8 digits) and the best of them, khat
hipError_t launch_bound_pass(gmmvb_workspace* ws, const EstepI8Args& a8, int is64, bool vec, hipStream_t st,
                             const char** name, int* rpw_out, int64_t* grid_out) {
    const int rpw = estep_i8_rows_per_wg();
    int64_t grid = (a8.n_rows + rpw - 1) / rpw;
    if (grid > (1 << 20)) grid = 1 << 20;
    *rpw_out = rpw;
    *grid_out = grid;
    EstepI8Args ab = a8;
    ab.img = ws->img_i8b;
    ab.khat = ws->khat;
    ab.ub = ws->ub32;           // the bounds go straight into the f32 array the sweeps carry
    return launch_estep_i8_bound(is64, vec, ws->bound.tb, (int)grid, st, ab, name);
}

// masks -> per-component lists -> chunk plan -> exact f64 evaluation of the listed pairs (all sized on the device)
hipError_t lists_and_gather(gmmvb_workspace* ws, const EstepArgs& a, int is64, bool vec, int sel_grid, hipStream_t st,
                            const float* thr = nullptr, const double* block_total = nullptr /*listed pairs per block, if counted*/) {
    if (thr) {
        hipError_t em = hipMemsetAsync(ws->exit_ctr, 0, sizeof(unsigned long long), st);
        if (em != hipSuccess) return em;
    }
    span_begin(ws, kSpanSelect, st);
    scan_and_fill(ws, st, ws->masks, ws->blk, sel_grid, a.n_rows, ws->K, block_total);
    hipLaunchKernelGGL(gather_plan_kernel, dim3(1), dim3(64), 0, st, ws->counts, ws->K,
                       estep_gather_rows_per_wg(ws->T, is64), ws->plan);
    hipError_t e = hipGetLastError();
    span_end(ws, st);
    if (e != hipSuccess) return e;
    span_begin(ws, kSpanGather, st);
    e = launch_estep_gather_dev(ws->T, is64, vec, 2 * ws->num_cu, st, a, ws->lists, ws->npad, ws->counts, ws->plan, thr,
                                thr ? ws->exit_ctr : nullptr, 0.0f);
    span_end(ws, st);
    ++ws->passes[7];
    return e;
}

}  // namespace

extern "C" {

// ---- pass policy: unit costs, thresholds and their calibration live in policy.h (ws->pt) --------------------------------

// Calibration of the policy table (policy.h) from the workspace's own passes: events around its first dense E-step, dense
// M-step and full bound pass of at least 2^23 pairs, taken over - like the pass counters - once they have completed.
bool cal_wanted(gmmvb_workspace* ws, int what, double pairs) {
    return ws->opt_calibrate && ws->cal_ev[0] != nullptr && !((ws->pt.measured >> what) & 1) && ws->cal_pairs[what] == 0.0 &&
           pairs >= (double)(int64_t(1) << 23) && ws->hmm == nullptr;
}
void cal_mark(gmmvb_workspace* ws, int what, double pairs, hipStream_t st) {
    note_hip(ws, hipEventRecord(ws->cal_ev[2 * what + 1], st));
    ws->cal_pairs[what] = pairs;
}
void cal_poll(gmmvb_workspace* ws) {
    for (int what = 0; what < 3; ++what) {
        if (ws->cal_pairs[what] <= 0.0 || hipEventQuery(ws->cal_ev[2 * what + 1]) != hipSuccess) continue;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ws->cal_ev[2 * what], ws->cal_ev[2 * what + 1]) == hipSuccess) {
            double ns = (double)ms * 1e6 / ws->cal_pairs[what];
            if (what == 2) ns += 0.010 * tri_pairs(ws->T) / 36.0;        // record building / selection around the bound kernel
            const bool took = ws->pt.take(what, ns);
            if (ws->opt_debug)
                std::fprintf(stderr, "[gmmvb] policy table: %s %.4f ns per pair %s (prune below %.3f, dense again above %.3f, list M below %.3f)\n",
                             what == 0 ? "dense E" : (what == 1 ? "dense M" : "bound pass"), ns, took ? "taken" : "out of range: literal kept",
                             ws->pt.prune_below(), ws->pt.dense_again_above(), ws->pt.list_m_below());
            if (!took) ws->pt.measured |= 8 << what;                     // (remembered as discarded: bits 3-5)
            // a discarded measurement (the process's first launch of a kernel pays its code upload; a small pass has a tail)
            // gets two more chances on later passes of the same kind
            ws->cal_pairs[what] = (took || ++ws->cal_tries[what] >= 3) ? -1.0 : 0.0;
        } else {
            ws->cal_pairs[what] = -1.0;
        }
    }
}

}  // extern "C"

namespace {

// The proof round over the lists just filled from the selection blocks' bases `blk_base`: by row superblocks when the item
// table fits the M-step's slabs (free during an E-step; estep_i8.h), else component after component.
hipError_t proof_round(gmmvb_workspace* ws, hipStream_t st, const int* blk_base, int sel_grid, int64_t n_rows, float* ub) {
    if (ws->opt_proof_blocked && ws->slabs &&
        estep_i8_proof_work_bytes(ws->K, n_rows) <= ws->scratch->bytes[kBuf_slabs])
        return launch_estep_i8_proof_blocked(ws->D, ws->num_cu, st, ws->xq, ws->xqe, ws->img_i8b, ws->cvec, ws->K, ws->lists,
                                             ws->npad, ws->counts, blk_base, sel_grid, ws->slabs, ub, ws->lnrho, ws->npad);
    hipLaunchKernelGGL(gather_plan_kernel, dim3(1), dim3(64), 0, st, ws->counts, ws->K, estep_i8_pairs_per_chunk(), ws->plan);
    return launch_estep_i8_proof(ws->D, ws->num_cu, st, ws->xq, ws->xqe, ws->img_i8b, ws->cvec, ws->K, ws->lists, ws->npad,
                                 ws->counts, ws->plan, ub, ws->lnrho, ws->npad);
}

// c_degree > 256 (generic.h): plain f64 kernels on the raw parameters, one dense pass and the rows' log-normalisers
int Pass::run_generic() {
    const int R = generic_rows(ws->D);
    const dim3 g((unsigned)((n_rows + R - 1) / R), (unsigned)ws->K);
    const size_t lds = (size_t)ws->D * R * sizeof(double);
    span_begin(ws, kSpanEstepMain, st);
    if (is64)
        hipLaunchKernelGGL(estep_generic_kernel<double>, g, dim3(64), lds, st, (const double*)x_dev, ldx, n_rows, ws->D,
                           ws->gen_u, ws->gen_m, ws->cvec, R, ws->lnrho, ws->npad);
    else
        hipLaunchKernelGGL(estep_generic_kernel<float>, g, dim3(64), lds, st, (const float*)x_dev, ldx, n_rows, ws->D,
                           ws->gen_u, ws->gen_m, ws->cvec, R, ws->lnrho, ws->npad);
    span_end(ws, st);
    if (phase_events(ws)) {          // (this path's E phase ends behind its main kernel)
        note_hip(ws, hipEventRecord(ws->ev[1], st));
        ws->ev_e = true;
    }
    phase_closed = true;
    span_begin(ws, kSpanLse, st);
    hipLaunchKernelGGL(row_lse_kernel, dim3((unsigned)((n_rows + kLseRows - 1) / kLseRows)), dim3(256), 0, st, ws->lnrho,
                       ws->npad, n_rows, ws->K, ws->lse, nullptr, nullptr, 1);
    span_end(ws, st);
    hipError_t eg = hipGetLastError();
    if (eg != hipSuccess) return fail(GMMVB_EHIP, "estep_generic launch", eg);
    ++ws->passes[0];
    ws->rec_live = ws->rec_valid = false;
    ws->evaluated = pairs;
    std::snprintf(ws->info, sizeof(ws->info), "estep_generic_f64<D=%d> grid=%ux%ux64 rows/workgroup=%d", ws->D, g.x, g.y, R);
    name = nullptr;
    return GMMVB_OK;
}

// every pair by one of the dense kernels, then the rows' log-normalisers - with the active pairs' masks and counts, and the
// records a pruned pass can start from, when the pass is large enough for either to matter
int Pass::run_dense() {
    const bool valu16 = ws->estep_variant == kEstepValu16 && ws->tri != nullptr;
    // an HMM pass that only the forward-backward recursions will read: rho' rows and row maxima straight into the HMM
    // state, no ln rho array (hmmvb_emission_target; hmm.h H0 + H1)
    emission_to_hmm = ws->T == 1 && !ws->wide && !i8 && !ws->sorted && hmm_fused_emission(ws->hmm);
    rpw = ws->wide ? estep_rows_rows_per_wg()
                     : (i8 ? estep_i8_rows_per_wg() : (valu16 ? estep_rows16_rows_per_wg() : estep_rows_per_wg(ws->estep_variant, ws->T, is64)));
    grid = (n_rows + rpw - 1) / rpw;
    if (grid > (1 << 20)) grid = 1 << 20;
    span_begin(ws, kSpanEstepMain, st);
    const bool cal_e = !ws->wide && !i8 && !emission_to_hmm && !valu16 && cal_wanted(ws, 0, pairs);
    if (cal_e) note_hip(ws, hipEventRecord(ws->cal_ev[0], st));
    hipError_t e = ws->wide ? launch_estep_rows(ws->T, is64, (int)grid, st, a, &name)
                            : (i8 ? launch_estep_i8(is64, vec, (int)grid, st, a8, &name)
                                  : (emission_to_hmm ? hmm_launch_emission16(ws->hmm, is64, vec, st, a, &name)
                                     : (valu16 ? launch_estep_rows16(is64, vec, (int)grid, st, a, ws->tri, &name)
                                            : launch_estep(ws->estep_variant, ws->T, is64, vec, (int)grid, st, a, &name))));
    if (cal_e) cal_mark(ws, 0, pairs, st);
    span_end(ws, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "estep launch", e);
    ++ws->passes[0];
    const int lse_blocks = (int)((n_rows + kLseRows - 1) / kLseRows);
    // small passes are launch-bound: no pair counting, no lists (the dense M-step takes microseconds there)
    const bool count_pairs = ws->sparse && ws->masks && ws->hmm == nullptr && n_rows * (int64_t)ws->K >= (int64_t(1) << 18);
    span_begin(ws, kSpanLse, st);
    if (count_pairs) {
        // thresholds from a sample of the rows (every 16th block of 1024), then lse + active masks + counts in one pass
        const int stride = lse_blocks >= 64 ? 16 : 1;
        const int sampled = (lse_blocks + stride - 1) / stride;
        hipLaunchKernelGGL(row_lse_kernel, dim3((unsigned)sampled), dim3(256), 0, st, ws->lnrho, ws->npad, n_rows, ws->K,
                           ws->lse, ws->dpart, nullptr, stride);
        hipLaunchKernelGGL(thr_kernel, dim3((unsigned)ws->K), dim3(256), 0, st, ws->dpart, nullptr, sampled, ws->K, ws->thr,
                           ws->ctr);
        hipLaunchKernelGGL(lse_mask_kernel, dim3((unsigned)sel_grid), dim3(kSelRows), 0, st, ws->lnrho, ws->npad, n_rows,
                           ws->K, ws->thr, ws->lse, ws->masks, ws->blk, ws->apart, ws->khat);
        hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(1024), 0, st, ws->apart, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, sel_grid, ws->ctr);
        // records for the next pass (one more sweep of the array, ~1 % of the dense kernel's time)
        if (prunable)
            hipLaunchKernelGGL(rec_build_kernel<false>, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, ws->lnrho,
                               ws->npad, n_rows, ws->K, ws->cvec, nullptr, rec, ws->ub32);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(GMMVB_EHIP, "row_lse / lse_mask launch", e);
        counted = true;
        ws->rec_valid = prunable;
    } else if (ws->hmm != nullptr) {
        // the HMM pass normalises along the time axis (hmm_prep_kernel takes the row maxima): the mixture's
        // log-normaliser is only made if a read-out asks for mixture responsibilities before hmmvb_forward_backward
        ws->lse_stale = true;
        ws->rec_valid = false;
    } else {
        hipLaunchKernelGGL(row_lse_kernel, dim3((unsigned)lse_blocks), dim3(256), 0, st, ws->lnrho, ws->npad, n_rows, ws->K,
                           ws->lse, nullptr, nullptr, 1);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(GMMVB_EHIP, "row_lse launch", e);
        ws->rec_valid = false;
    }
    span_end(ws, st);
    ws->rec_live = false;
    ws->evaluated = pairs;
    return GMMVB_OK;
}

// Bound pass: int8 upper bounds of every pair, the best component of every row exactly, records from both, and - when the
// proof round is available - the candidates through it before the exact gather.  Leaves the select span's masks and counts
// for run_candidates().
int Pass::run_bound() {
    span_begin(ws, kSpanEstepMain, st);
    // (only a pass over all output blocks measures what the table's bound_ns stands for)
    const bool cal_b = ws->bound.tb == (ws->D + 31) / 32 && cal_wanted(ws, 2, pairs);
    if (cal_b) note_hip(ws, hipEventRecord(ws->cal_ev[4], st));
    hipError_t e = launch_bound_pass(ws, a8, is64, vec, st, &name, &rpw, &grid);
    if (cal_b) cal_mark(ws, 2, pairs, st);
    span_end(ws, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "estep_bound launch", e);
    ++ws->passes[1];
    // the best component of every row, exactly
    span_begin(ws, kSpanSelect, st);
    hipLaunchKernelGGL(select_mask_kernel<3>, dim3(sel_grid), dim3(kSelRows), 0, st, ws->lnrho, ws->npad, n_rows, ws->K, ws->khat,
                       ws->masks, ws->blk);
    span_end(ws, st);
    e = lists_and_gather(ws, a, is64, vec, sel_grid, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "E-step best-component evaluation", e);
    // records from the bounds (+ the one exact value), then every other candidate
    span_begin(ws, kSpanSelect, st);
    hipLaunchKernelGGL(rec_build_kernel<true>, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, ws->lnrho, ws->npad,
                       n_rows, ws->K, ws->cvec, ws->khat, rec, ws->ub32);
    hipLaunchKernelGGL(rec_select_kernel, dim3(sel_grid), dim3(kSelRows), 0, st, rec, n_rows, ws->K, ws->cvec, ws->masks,
                       ws->npad, ws->blk, ws->epart, ws->opart, ws->rthr);
    if (proof_capable) {
        // the candidates' bounds come from the bound pass's leading output blocks only: three int8 digits over ALL
        // blocks first (a third of an exact evaluation's cost), and only what still does not clear the threshold
        // goes to the exact gather
        scan_and_fill(ws, st, ws->masks, ws->blk, sel_grid, n_rows, ws->K, ws->epart);
        span_end(ws, st);
        span_begin(ws, kSpanProof, st);
        e = proof_round(ws, st, ws->blk, sel_grid, n_rows, ws->ub32);
        span_end(ws, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "proof round (bound pass)", e);
        span_begin(ws, kSpanSelect, st);
        hipLaunchKernelGGL(rec_prune_kernel, dim3(sel_grid), dim3(kSelRows), 0, st, rec, ws->masks, ws->npad, n_rows, ws->K,
                           ws->cvec, ws->ub32, ws->rthr, ws->blk, ws->epart, ws->ppart);
        proof_ran = true;
    }
    span_end(ws, st);
    return GMMVB_OK;
}

// The sweep of the carried bounds itself, over rows whose reference values (the previous pass's active pairs) are exact under
// the parameters in force: stateless from the table of project.h, lazy over the tile state, or through all K bounds.
// Inside the caller's select span.
int Pass::sweep_bounds(bool proof, bool own_round) {
    unsigned char* lock = settle ? ws->lock : nullptr;
    unsigned long long* pmask = proof ? ws->rmask : nullptr;
    const int proof_all = ws->opt_proof_all ? 1 : 0, own_fresh = own_round ? 1 : 0;
    // the tile state (workspace.h) is kept by the carried forms only, and not next to the table's filter
    int* tile_loose = can_project ? nullptr : ws->tile_loose();
    unsigned long long* quiet_ctr = (tile_loose && ws->opt_debug) ? ws->exit_ctr + 3 : nullptr;
    if (quiet_ctr) note_hip(ws, hipMemsetAsync(quiet_ctr, 0, sizeof(unsigned long long), st));
    if (can_project && ws->opt_project == 2) {
        // bounds from the table of the parameters in force and the rows' digit planes: nothing carried, nothing
        // written back (the per-pair array is void afterwards: ws->dense_valid in finish())
        note_hip(ws, hipMemsetAsync(ws->exit_ctr + 2, 0, sizeof(unsigned long long), st));
        hipError_t e = launch_rec_project(sel_grid, st, project_args(ws, n_rows, lock, pmask, proof_all, own_fresh));
        if (e != hipSuccess) return fail(GMMVB_EHIP, "rec_project launch", e);
        name = "estep_sweep_projected";
        projected = true;
    } else if (ws->tmeta) {
        note_hip(ws, hipMemsetAsync(ws->exit_ctr + 1, 0, sizeof(unsigned long long), st));
        // (the tile state is void after any pass that rewrote the bounds wholesale: the first sweep after it
        // opens every column and takes stock)
        const int run = sweep_run_length(ws->K, ws->opt_sweep_run);
        dispatch_mask_words(ws->K, [&](auto wc) {        // (mask words and run length as compile-time constants)
            dispatch_sweep_run(run, [&](auto rr) {
                constexpr int WC = decltype(wc)::value, R = WC <= 2 ? decltype(rr)::value : 1;
                hipLaunchKernelGGL((rec_sweep_kernel<true, true, WC, R>), dim3((sel_grid + R - 1) / R), dim3(kSelRows), 0, st,
                                   ws->ub32, ws->lnrho, ws->npad, n_rows, ws->K, ws->drift, ws->cvec, ws->khat, rec, ws->masks,
                                   ws->blk, ws->epart, ws->opart, lock, ws->dlock, ws->rthr, ws->lcomp, pmask, ws->rblk, proof_all,
                                   own_fresh, ws->tmeta, tmeta_was_valid ? 0 : 1, ws->exit_ctr + 1, ws->ppart, tile_loose, quiet_ctr);
            });
        });
        tmeta_kept = true;
        quiet_swept = tile_loose != nullptr;
    } else {
        hipLaunchKernelGGL(rec_sweep_kernel<true>, dim3(sel_grid), dim3(kSelRows), 0, st, ws->ub32, ws->lnrho, ws->npad, n_rows,
                           ws->K, ws->drift, ws->cvec, ws->khat, rec, ws->masks, ws->blk, ws->epart, ws->opart, lock, ws->dlock,
                           ws->rthr, ws->lcomp, pmask, ws->rblk, proof_all, own_fresh, nullptr, 0, nullptr, ws->ppart, tile_loose,
                           quiet_ctr);
        quiet_swept = tile_loose != nullptr;
    }
    return GMMVB_OK;
}

// Sweep whose round 0 evaluates the previous pass's lists - every pair that was active - as they are: the M-step's lists
// are still in the workspace with their masks (no list building), or are rebuilt from the masks and block counts.
int Pass::run_sweep_over_lists() {
    span_begin(ws, kSpanSelect, st);
    if (!ws->active_lists)          // (the M-step's lists left out the rows in its cache)
        // (gpart: the listed pairs rec_finish_kernel counted per block when it wrote these masks)
        scan_and_fill(ws, st, ws->masks, ws->blk, sel_grid, n_rows, ws->K, ws->prev_pass != 0 ? ws->gpart : nullptr);
    hipLaunchKernelGGL(gather_plan_kernel, dim3(1), dim3(64), 0, st, ws->counts, ws->K, estep_gather_rows_per_wg(ws->T, is64),
                       ws->plan);
    span_end(ws, st);
    span_begin(ws, kSpanGather, st);
    hipError_t e = launch_estep_gather_dev(ws->T, is64, vec, 2 * ws->num_cu, st, a, ws->lists, ws->npad, ws->counts, ws->plan);
    span_end(ws, st);
    ++ws->passes[7];
    if (e != hipSuccess) return fail(GMMVB_EHIP, "E-step active-pair evaluation", e);
    const bool proof = proof_capable && (ws->skip_used || ws->opt_proof_all);       // (some rows may be settled)
    // Settled rows of components that moved noticeably: a fresh lower bound of their own pair first (three int8
    // digits), so that the sweep compares the other components' bounds with a tight reference instead of one
    // carried through Gamma and delta (records.h, own_first).  While the summary of the drift says that no
    // component moves that much the round is skipped altogether.
    const bool own_round = proof && ws->skip_used && !(ws->typical_gamma >= ws->pt.own_round_below);
    if (own_round) {
        span_begin(ws, kSpanSelect, st);
        hipLaunchKernelGGL(settled_mask_kernel, dim3(sel_grid), dim3(kSelRows), 0, st, ws->lock, ws->masks, ws->lcomp, ws->npad,
                           n_rows, ws->K, ws->rmask, ws->rblk, ws->drift, ws->spart, quiet_was_valid ? ws->tile_quiet() : nullptr);
        scan_and_fill(ws, st, ws->rmask, ws->rblk, sel_grid, n_rows, ws->K, ws->spart);
        span_end(ws, st);
        span_begin(ws, kSpanProof, st);
        e = proof_round(ws, st, ws->rblk, sel_grid, n_rows, nullptr);
        span_end(ws, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "proof round (settled rows' own pairs)", e);
    }
    span_begin(ws, kSpanSelect, st);
    int rc = sweep_bounds(proof, own_round);
    if (rc) return rc;
    if (proof && can_project && !projected) {
        // the table of the parameters in force first (project.h): a listed pair it clears needs no proof - most of
        // them are far pairs whose carried bound has eroded to the relevance line
        note_hip(ws, hipMemsetAsync(ws->exit_ctr + 2, 0, sizeof(unsigned long long), st));
        e = launch_proj_filter(sel_grid, st, project_args(ws, n_rows, ws->lock, ws->rmask, 0, 0));
        if (e != hipSuccess) return fail(GMMVB_EHIP, "proj_filter launch", e);
        filtered = true;
    }
    if (proof) {
        // proof round: settled rows whose carried bounds left candidates - their component and the candidates
        // get two-sided bounds from three int8 digits; rows that are proven stay settled, the others join
        // the pass's lists (records.h)
        // (ppart: the proof pairs the sweep listed per block; rec_proof_decide_kernel overwrites it afterwards)
        scan_and_fill(ws, st, ws->rmask, ws->rblk, sel_grid, n_rows, ws->K, projected ? nullptr : ws->ppart);
        span_end(ws, st);
        span_begin(ws, kSpanProof, st);
        e = proof_round(ws, st, ws->rblk, sel_grid, n_rows, ws->ub32);
        span_end(ws, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "proof round", e);
        span_begin(ws, kSpanSelect, st);
        hipLaunchKernelGGL(rec_proof_decide_kernel, dim3(sel_grid), dim3(kSelRows), 0, st, rec, ws->rmask, ws->masks, ws->npad,
                           n_rows, ws->K, ws->cvec, ws->ub32, ws->lnrho, ws->lcomp, ws->dlock, ws->rthr, ws->blk, ws->epart,
                           ws->ppart, own_round ? ws->spart : nullptr, quiet_swept ? ws->tile_loose() : nullptr);
        proof_ran = true;
    }
    span_end(ws, st);
    return GMMVB_OK;
}

// Sweep without the previous pass's lists (another tile of the group used the buffers, or the pass before was not counted):
// round 0 evaluates the previous best component of every row.
int Pass::run_sweep_from_best() {
    span_begin(ws, kSpanSelect, st);
    hipLaunchKernelGGL(select_mask_kernel<3>, dim3(sel_grid), dim3(kSelRows), 0, st, ws->lnrho, ws->npad, n_rows, ws->K, ws->khat,
                       ws->masks, ws->blk);
    span_end(ws, st);
    hipError_t e = lists_and_gather(ws, a, is64, vec, sel_grid, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "E-step best-component evaluation", e);
    span_begin(ws, kSpanSelect, st);
    hipLaunchKernelGGL(rec_sweep_kernel<false>, dim3(sel_grid), dim3(kSelRows), 0, st, ws->ub32, ws->lnrho, ws->npad, n_rows, ws->K,
                       ws->drift, ws->cvec, ws->khat, rec, ws->masks, ws->blk, ws->epart, ws->opart,
                       settle ? ws->lock : nullptr, ws->dlock, ws->rthr, ws->lcomp, nullptr, nullptr, 0, 0, nullptr, 0);
    span_end(ws, st);
    return GMMVB_OK;
}

// Sweep: round 0 evaluates exactly, under the new parameters, the pairs the sweep takes its reference values from; then
// every carried bound moves with its component's drift and what no longer clears the row's threshold becomes a candidate.
int Pass::run_sweep() {
    rpw = kSelRows;
    grid = sel_grid;
    name = "estep_sweep_bounds";
    ++ws->passes[4];
    ++ws->sweeps;
    const int rc = prev_lists ? run_sweep_over_lists() : run_sweep_from_best();
    if (rc) return rc;
    ws->sweep_prev = prev_lists;
    return GMMVB_OK;
}

// What a bound pass and a sweep end in: the exact evaluation of the candidates they listed, then the records' final word on
// every row (log-normaliser, active masks, the M-step's and the cache's delta masks) and the pass's counters.
int Pass::run_candidates() {
    // candidates: a pair whose first output blocks already put it below the row's threshold is not evaluated further
    hipError_t e = lists_and_gather(ws, a, is64, vec, sel_grid, st, ws->gather_exit ? ws->rthr : nullptr, ws->epart);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "E-step candidate evaluation", e);
    span_begin(ws, kSpanLse, st);
    hipLaunchKernelGGL(rec_finish_kernel, dim3(sel_grid), dim3(kSelRows), 0, st, rec, ws->lnrho, ws->npad, n_rows, ws->K,
                       ws->cvec, ws->lse, ws->khat, ws->masks, ws->blk, ws->apart, ws->mpart, ws->ub32,
                       settle ? ws->lock : nullptr, ws->dlock, skip_margin, settle ? ws->dmask : nullptr,
                       settle ? ws->dblk : nullptr, ws->mmask, ws->mblk, ws->spart, ws->gpart, ws->qpart, ws->rthr, ws->lcomp,
                       quiet_swept ? ws->tile_loose() : nullptr, quiet_swept ? ws->tile_quiet() : nullptr, quiet_was_valid ? 1 : 0,
                       (quiet_swept && ws->opt_debug) ? ws->exit_ctr + 3 : nullptr);
    if (!proof_ran) note_hip(ws, hipMemsetAsync(ws->ctr + 7, 0, sizeof(double), st));
    hipLaunchKernelGGL(sum_parts_kernel, dim3(proof_ran ? 8 : 7), dim3(1024), 0, st, ws->apart, ws->epart, ws->opart, ws->mpart,
                       ws->spart, ws->gpart, ws->qpart, ws->ppart, sel_grid, ws->ctr);
    e = hipGetLastError();
    span_end(ws, st);
    if (e != hipSuccess) return fail(GMMVB_EHIP, "rec_finish launch", e);
    counted = true;
    ws->rec_valid = true;
    ws->rec_live = true;
    ws->evaluated = -1.0;
    ws->quiet_valid = quiet_swept;     // (rec_finish_kernel has just written tile_quiet for every tile)
    if (settle) {
        ws->lock_live = true;
        ws->delta_pending = true;
    }
    return GMMVB_OK;
}

// The tail every pass goes through: the end of the profile's E phase, the counters' copy to the host, and every field the
// M-step, the read-outs and the next E-step read to know what happened.  (A generic workspace goes through it too: the
// fields its own tail never wrote - the lazy sweep's and the table's flags, pol.valid, act_host, the list flags, blk_fresh,
// hmm_no_lnrho, bounds_*, dense_valid, sweeps - are read by passes and read-outs it does not have, and all but bounds_* and
// dense_valid keep the value they had.)
int Pass::finish(const char* latch_what) {
    ws->tmeta_valid = tmeta_kept;
    ws->pend_lazy = tmeta_kept;
    ws->pend_proj = projected || filtered;
    ws->pend_quiet = quiet_swept && ws->opt_debug;
    // the E phase of the profile ends behind the pass's LAST kernel (round 4; before, rec_finish / lse_mask - 0.2-0.4 ms of
    // E-step work at the benchmark shape - fell between the two phases and were booked as "outside the data pass")
    if (!phase_closed && phase_events(ws)) {
        note_hip(ws, hipEventRecord(ws->ev[1], st));
        ws->ev_e = true;
    }
    // counters -> pinned host memory, behind an event (read by the next pass, or by gmmvb_last_sparsity)
    if (counted) {
        hipError_t e = hipMemcpyAsync(ws->ctr_host, ws->ctr, 8 * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && ws->exit_ctr && mode != kPassDense)
            e = hipMemcpyAsync(ws->exit_host, ws->exit_ctr, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(ws->ctr_ev, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "E-step counters", e);
        ws->ctr_pending = true;
        ws->pend_mode = mode;
        ws->pend_rows = n_rows;
        // pairs evaluated before the counted selection: every row's best component, or (sweep over the previous
        // pass's lists) the previous pass's active pairs
        ws->pend_first_sorted = sorted_now;
        ws->pend_round0 = (mode == kPassSweep && ws->sweep_prev && own_known) ? ws->lag.listed : (double)n_rows;
        ws->act_rows = n_rows;
    } else {
        ws->ctr_pending = false;
        ws->lag.valid = false;
        ws->act_rows = 0;              // nothing counted: dense M-step, no pruning decision from this pass
    }
    ws->exp_counted = counted;
    ws->pol.valid = false;             // (a sharded job imports this pass's sums before the next E-step)
    ws->act_host = -1.0;
    ws->active_lists = false;
    ws->mlists_done = ws->mlists_lost = false;
    if (skip_margin >= 0.0) ws->skip_used = true;
    ws->blk_fresh = counted;
    ws->e_state = emission_to_hmm ? 4 : 1;
    ws->hmm_no_lnrho = emission_to_hmm;
    ws->lost_estep = false;
    ws->e_rows = n_rows;
    ws->params_used = true;
    ws->have_drift = false;
    ws->bounds_rows = n_rows;          // the records / the ln rho array now belong to the parameters in force, on these rows
    ws->bounds_x = x_dev;
    ws->bounds_ldx = ldx;
    ws->prev_pass = mode;
    // the f32 bound array holds a value or bound under the parameters in force for EVERY pair after a dense pass, a
    // bound pass or a sweep; a pass on records only refreshes the evaluated entries
    // (a projected sweep leaves the array alone: it is void until a dense or bound pass rewrites it)
    ws->dense_valid = !projected;
    if (mode == kPassDense || mode == kPassBound) ws->sweeps = 0;
    if (name)
        std::snprintf(ws->info, sizeof(ws->info), "%s grid=%lldx%d rows/workgroup=%d", name, (long long)grid,
                      (i8 || mode != kPassDense) ? 512 : estep_threads(ws->estep_variant), rpw);
    return take_hip(ws, latch_what);
}

// What choose_pass reads (pass_plan.h), from the workspace and this call's matrix.  Fills the pass's own copies of the
// facts its launches need as well.
PassFacts Pass::facts() {
    PassFacts f;
    f.L = ws->sharded ? ws->pol : ws->lag;
    f.prune = ws->prune;
    f.xc_of_x = xc_is_of(ws, x_dev, ldx, n_rows);
    f.has_xc = ws->xc != nullptr;
    f.can_prune = ws->prune != 0 && ws->estep_variant == kEstepLds8 && ws->hmm == nullptr && ws->rec_k != nullptr && f.has_xc &&
                  f.xc_of_x;
    const int64_t size_rows = ws->sharded ? ws->shard_rows / ws->shard_ranks : n_rows;
    f.big = ws->prune == 2 || size_rows * (int64_t)ws->K >= (int64_t(1) << 23);
    f.same_rows = ws->bounds_rows == n_rows && ws->bounds_x == x_dev && ws->bounds_ldx == ldx;
    // counters of the previous pass, over rows_l rows (this rank's, or the job's)
    f.known = f.L.valid && (ws->sharded || (f.L.rows == (double)n_rows && !ws->ctr_pending));
    // (this rank's own numbers of the previous pass: what its kernels did)
    own_known = ws->lag.valid && ws->lag.rows == (double)n_rows && !ws->ctr_pending;
    // the previous pass's M-step left its per-component lists of active rows (and their masks) in the workspace
    // (or the masks and block counts they are built from)
    // (an E-step whose output went to another tile of the group still left its masks, block counts and best components)
    f.after_estep = ws->e_state == 1 || ws->lost_estep;
    f.prev_lists = (ws->active_lists || ws->blk_fresh) && f.after_estep && ws->act_rows == n_rows && f.same_rows;
    f.xq_of_x = xq_is_of(ws, x_dev, ldx, n_rows);
    // The stateless sweep (project.h) needs no carried per-pair bounds: the table gmmvb_set_params made for these parameters,
    // the digit planes of this matrix about the pivot in force, regrouped rows and the previous pass's lists.
    f.can_project = ws->proj_table && ws->gimg != nullptr && ws->sorted && ws->tile_ref_valid && f.prev_lists && f.xq_of_x &&
                    ws->xq_gen == ws->pivot_gen && ws->lock != nullptr;
    f.forget = ws->forget;
    f.have_drift = ws->have_drift;
    f.opt_carry_off = ws->opt_carry_off;
    f.dense_valid = ws->dense_valid;
    f.opt_project = ws->opt_project;
    f.typical_gamma = ws->typical_gamma;
    f.bound_fail_act = ws->bound_fail_act;
    f.bound_tb = ws->bound.tb;
    f.T = ws->T, f.K = ws->K, f.D = ws->D;
    f.n_rows = n_rows;
    f.sort_rows = ws->sort_rows, f.has_xp = ws->xp != nullptr, f.sorted = ws->sorted;
    f.sorts = ws->sorts;
    f.moved_since_sort = ws->moved_since_sort;
    f.hmm = ws->hmm != nullptr;
    f.has_lock = ws->lock != nullptr, f.lock_reset = ws->lock_reset, f.lock_live = ws->lock_live;
    f.delta_pending = ws->delta_pending, f.cache_on = ws->cache_on, f.sparse = ws->sparse, f.has_masks = ws->masks != nullptr;
    f.opt_proof = ws->opt_proof, f.has_bound_images = ws->img_i8b != nullptr, f.xq_current = ws->xq_gen == ws->img_gen;
    f.settle_margin = ws->settle_margin;
    prunable = f.can_prune && f.big;
    prev_lists = f.prev_lists;
    can_project = f.can_project;
    return f;
}

// The plan's effects on the workspace before anything is launched (in the order the decision used to take them).
int Pass::apply(const PassFacts& f, const PassPlan& plan) {
    if (plan.spare_set) ws->spare_last = plan.spare_last;
    if (plan.fell_back) ++ws->passes[3];
    ws->bound_fail_act = plan.bound_fail_act;
    ws->forget = false;
    if (ws->lock) {
        if (plan.reset_cache) {
            // (a failed reset would leave stale addends in the cache: the pass must not go on)
            hipError_t e = hipMemsetAsync(ws->lock, 0, (size_t)ws->npad, st);
            if (e == hipSuccess) e = hipMemsetAsync(ws->cache, 0, (size_t)gmmvb_stats_len(ws->K, ws->D) * sizeof(double), st);
            if (e != hipSuccess) return fail(GMMVB_EHIP, "resetting the cache of single-component rows", e);
            ws->lock_live = false;
            ws->skip_used = false;
            ws->quiet_valid = false;
        }
        ws->lock_reset = false;
        ws->delta_pending = false;
    }
    ws->settled_fresh = false;
    mode = plan.mode;
    settle = plan.settle;
    proof_capable = plan.proof_capable;
    skip_margin = plan.skip_margin;
    if (ws->opt_debug) {
        const gmmvb_pass_counters& L = f.L;
        const double rows_l = f.rows_l();
        // (quiet: tiles the lag pass's sweep left without a loose row, of its tiles; skipped: tiles rec_finish_kernel did not
        // go through row by row - quiet there too, after the proof round, and in the pass before; -1: no tile state kept)
        std::fprintf(stderr, "[gmmvb] estep: mode=%d known=%d lag(mode=%d act=%.3g eval=%.3g over=%.3g settled=%.3g listed=%.3g) gamma=%.3f rec_valid=%d drift=%d settle=%d quiet=%.0f/%lld skipped=%.0f\n",
                     plan.mode, (int)f.known, L.mode, L.act / rows_l, L.eval / rows_l, L.over / rows_l, L.settled / rows_l,
                     L.listed / rows_l, ws->typical_gamma, (int)ws->rec_valid, (int)ws->have_drift, (int)plan.settle,
                     ws->lag.valid ? ws->lag_quiet : -1.0, (long long)((n_rows + kSelRows - 1) / kSelRows),
                     ws->lag.valid ? ws->lag_skipped : -1.0);
    }
    // (the caller hands over drift hints - a row-tiled pass, whose bounds do not survive the other tiles, does not)
    const bool wants_drift = gmmvb_wants_drift(ws, n_rows) != 0;
    ws->bound.choose(plan.mode, ws->img_i8b != nullptr, f.L, f.known, wants_drift && ws->have_drift, wants_drift, ws->pt, ws->T,
                     ws->D, ws->K);
    return GMMVB_OK;
}

}  // namespace

extern "C" {

int gmmvb_estep(gmmvb_workspace* ws, const void* x_dev, int64_t ldx, int64_t n_rows, void* stream) {
    bool vec = false;
    int rc = check_x(ws, x_dev, ldx, n_rows, &vec);
    if (rc) return rc;
    if (!ws->have_params) return fail(GMMVB_ESTATE, "gmmvb_set_params has not been called");
    claim_scratch(ws);
    hipStream_t st = (hipStream_t)stream;
    Pass p{ws, x_dev, ldx, n_rows, st, ws->x_dtype == GMMVB_F64, vec, (int)((n_rows + kSelRows - 1) / kSelRows),
           (double)n_rows * ws->K};
    if (ws->generic) {
        if (phase_events(ws)) note_hip(ws, hipEventRecord(ws->ev[0], st));
        ws->n_spans = 0;
        rc = p.run_generic();
        return rc ? rc : p.finish("event record inside the E-step");
    }
    p.i8 = ws->estep_variant == kEstepI8;
    p.a = EstepArgs{x_dev, ldx, n_rows, ws->D, ws->img, ws->cvec, ws->K, ws->lnrho, ws->npad};
    p.a8 = EstepI8Args{x_dev, ldx, n_rows, ws->D, ws->img_i8, ws->pivot_i8, ws->cvec, ws->K, ws->lnrho, ws->npad};
    if (ws->sorted && ws->xc_src != x_dev) ws->sorted = false;      // another matrix: the caller's order

    // ---- which kind of pass?  (pass_plan.h)
    if (ws->sharded) {
        rc = take_policy(ws);
        if (rc) return rc;
    }
    poll_counters(ws);
    cal_poll(ws);
    const PassFacts facts = p.facts();
    const PassPlan plan = choose_pass(ws->pt, facts);
    rc = p.apply(facts, plan);
    if (rc) return rc;

    if (phase_events(ws)) note_hip(ws, hipEventRecord(ws->ev[0], st));
    ws->n_spans = 0;
    if (plan.regroup) {
        span_begin(ws, kSpanSelect, st);
        hipError_t e = regroup_rows(ws, x_dev, ldx, n_rows, st, ws->lock_live, ws->e_state == 1 && !ws->lse_stale);
        span_end(ws, st);
        if (e != hipSuccess) return fail(GMMVB_EHIP, "regrouping the rows", e);
        ws->moved_since_sort = 0.0;
        p.sorted_now = true;
    }
    if (ws->sorted) {           // the kernels read the workspace's permuted copy
        p.a.x = p.a8.x = ws->xp;
        p.a.ldx = p.a8.ldx = ws->D;
        p.vec = ws->D % 16 == 0;
    }
    p.rec = RecArrays{ws->rec_k, ws->rec_d, ws->rec_B, ws->rec_exact, ws->rec_sel, ws->rec_flags, ws->npad};
    ws->lse_stale = false;
    p.tmeta_was_valid = ws->tmeta_valid;
    ws->tmeta_valid = false;            // (only a lazy sweep that ran to its end leaves the tile state in step with the bounds)
    p.quiet_was_valid = ws->quiet_valid && !plan.regroup && ws->tile_quiet() != nullptr;
    ws->quiet_valid = false;            // (only a counted sweep that ran to its end leaves the settled rows' tile state valid)
    if (p.mode == kPassDense) {
        rc = p.run_dense();
    } else {
        rc = p.mode == kPassBound ? p.run_bound() : p.run_sweep();
        if (rc == GMMVB_OK) rc = p.run_candidates();
    }
    return rc ? rc : p.finish("event record / counter reset inside the E-step");
}

}  // extern "C"
