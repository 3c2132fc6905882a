// Which kind of pass the next E-step is (dense, bound pass or sweep), and how many output blocks a bound pass evaluates.
//
// Decided from what the host knows WITHOUT waiting for the device: the counters of the last E-step whose copy has arrived
// (they lag by one pass when the caller never synchronises; results do not depend on the choice, only the time does).
// A shard of a row-sharded job (gmmvb_set_shard) decides from the counters summed over all ranks and from the job's size -
// nothing here differs between ranks, so neither do the decisions.
//
// Plain C++: gmmvb_estep (capi_estep.hip) fills PassFacts from the workspace, calls choose_pass and BoundLevel::choose and
// applies the plan; tests/pass_plan_cases.cpp drives the same two functions from a host compiler.  No HIP header here.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "policy.h"

// What an E-step leaves for the policy of the next one (and for gmmvb_last_work)
struct gmmvb_pass_counters {
    bool valid = false;
    double act = 0.0, eval = 0.0, over = 0.0, settled = 0.0, listed = 0.0, accum = 0.0, proof = 0.0, exits = 0.0, moved = 0.0;
    double cols = -1.0;          // (tile, component) columns of the bound array the last sweep went through; -1: not a lazy sweep
    double left = -1.0;          // pairs the stateless table (project.h) did not clear; -1: the pass was no projected sweep
    double rows = 0.0;           // rows the counters were taken over
    double ranks = 1.0;          // ranks they were summed over
    int mode = 0;                // kind of the pass: 0 dense, 1 bound pass, 2 carried records, 3 sweep
};

namespace gmmvb {

enum { kPassDense = 0, kPassBound = 1, kPassSweep = 3 };      // (2 was the pass on per-row records, gone in round 3)

// Everything the decision reads, as values.
struct PassFacts {
    gmmvb_pass_counters L;           // counters of the previous pass (this rank's, or the job's)
    bool known = false;              // ... have arrived, over these rows
    // (a pruned E-step leaves exact ln rho for the listed pairs only, so its M-step has to run over the lists - which read
    // the rows through the workspace's prepared copy: without gmmvb_prepare_rows for this matrix the pass stays dense)
    bool can_prune = false;
    bool big = false;                // GMMVB_ESTEP_PRUNE=force, or at least 2^23 pairs
    int prune = 1;                   // 0 never, 1 by the policy, 2 forced
    bool forget = false;             // gmmvb_forget: the parameters are unrelated to the last E-step's
    bool same_rows = false;          // the bounds / records belong to this matrix
    bool after_estep = false;        // the last call left E-step output (here, or with another tile of the group)
    bool prev_lists = false;         // the previous pass's lists (or their masks and block counts) are in the workspace
    bool have_drift = false, opt_carry_off = false, dense_valid = false, can_project = false;
    int opt_project = 0;
    double typical_gamma = -1.0;
    double bound_fail_act = -1.0;
    int bound_tb = 0;
    int T = 0, K = 0, D = 0;
    int64_t n_rows = 0;
    // regrouping
    bool sort_rows = false, has_xp = false, sorted = false;
    int64_t sorts = 0;
    double moved_since_sort = 0.0;
    bool has_xc = false, xc_of_x = false;      // the centred copy exists / is of this matrix
    bool hmm = false;
    // cache of settled rows
    bool has_lock = false, lock_reset = false, lock_live = false, delta_pending = false, cache_on = false, sparse = false,
         has_masks = false;
    // proof round: the digit planes are of this matrix, about the pivot the 3-digit images were packed for
    bool opt_proof = false, xq_of_x = false, has_bound_images = false, xq_current = false;
    double settle_margin = 1e300;

    double rows_l() const { return known ? L.rows : (double)n_rows; }      // rows the counters were taken over
    double pairs_l() const { return rows_l() * K; }
};

// Everything the decision produces.
struct PassPlan {
    int mode = kPassDense;
    bool fell_back = false;          // a pruned E-step that went back to the dense kernel (gmmvb_pass_counts)
    double bound_fail_act = -1.0;    // the workspace's new value
    bool spare_set = false;          // spare_last was worked out (diagnostics: the workspace keeps its old value otherwise)
    double spare_last = -1.0;
    bool regroup = false;            // regroup the rows by best component before this (bound) pass
    bool reset_cache = false;        // empty the cache of single-component rows first
    bool settle = false;             // rows with one active component may be settled
    bool proof_capable = false;      // the proof round is available
    double skip_margin = -1.0;       // nats of slack demanded of a row that settles (< 0: none settles)
};

inline PassPlan choose_pass(const PolicyTable& pt, const PassFacts& f) {
    PassPlan p;
    p.bound_fail_act = f.bound_fail_act;
    int mode = kPassDense;
    const gmmvb_pass_counters& L = f.L;
    const bool known = f.known;
    const double rows_l = f.rows_l(), pairs_l = f.pairs_l();
    if (f.can_prune && f.big) {
        // sparse enough?  (never for an HMM workspace: forward-backward consumes every emission ln rho)
        bool sparse_ok = f.prune == 2;
        if (!sparse_ok && known && !f.forget) sparse_ok = L.act <= pt.prune_below() * pairs_l;
        // a bound pass that left most pairs candidates (below) is not tried again until a quarter fewer pairs are active than
        // when it failed: at cluster spread 0.75 (31-40 of 64 active for twenty passes) every other pass was such an attempt
        if (sparse_ok && f.prune != 2 && known && f.bound_fail_act > 0.0 && L.act > 0.75 * f.bound_fail_act * pairs_l)
            sparse_ok = false;
        if (sparse_ok) {
            mode = kPassBound;
            const bool hinted = f.same_rows && f.have_drift && !f.opt_carry_off;
            // Carrying the previous pass over the parameter update (gmmvb_set_drift): a sweep of the f32 per-pair bound
            // array, every entry with its own component's drift (1.5 ms at C3), after the previous pass's active pairs have
            // been evaluated under the new parameters.  (Round 2 also had a pass on 55-byte per-row records with ONE rest
            // bound per row; it eroded at the pace of the fastest-moving component and the default policy never chose it.)
            // typical_gamma is the caller's pessimistic summary min_k (gamma_k - delta_k / 30) (0.3, 0.6, 0.7, 0.8 in
            // the first iterations at C3, 0.94 by the 13th, 0.97 by the 20th, 0.99 by the 26th): below 0.5 the bounds are
            // made afresh.
            const double tg = f.typical_gamma;
            bool sweep = hinted && (f.dense_valid || (f.can_project && f.opt_project == 2)) && !(tg > 0.0 && tg < pt.gamma_no_carry);
            if (sweep && known && L.mode != kPassDense) {
                // spare candidates (listed but inactive) of the last pruned pass: carry on only while evaluating them
                // (they grow from pass to pass) costs less than a fresh bound pass, and while few rows overflow
                // (a pair of the proof round costs about a third of an exact evaluation)
                // (a bound pass's own proof stage works through the candidates its coarse bounds leave - not a sign of erosion)
                const double spare = (std::max(0.0, L.eval - (L.act - L.settled)) + (L.mode == kPassSweep ? pt.proof_per_exact * L.proof : 0.0)) / pairs_l;
                p.spare_set = true;
                p.spare_last = spare;
                const int tb = f.bound_tb > 0 ? f.bound_tb : 3;
                const double bound_cost = pt.i8_block_pair * tri_pairs(tb) + pt.i8_row_of_y * 32 * tb, gpp = pt.f64_tile_pair * tri_pairs(f.T);
                if (gpp * spare * pt.spare_growth >= bound_cost) sweep = false;
                // rows whose record had to be rebuilt in full cost K evaluations each and multiply from pass to pass
                // (x4 - x8 observed): stop carrying well before they dominate
                if (L.over > pt.overflow_rows * rows_l || L.eval > pt.carried_eval_above * pairs_l) sweep = false;
            }
            if (sweep && known && L.mode == kPassDense && L.act > pt.sweep_after_dense_below * pairs_l) sweep = false;
            // straight from a dense pass the parameters usually still jump (second or third iteration of a restart): the
            // sweep's per-pair bounds are exact values then, but carried over such an update most of them end up
            // candidates (measured at C4: 118 of 256 per row, 171 ms) - a bound pass is the safe first pruned pass
            if (sweep && known && L.mode == kPassDense && tg > 0.0 && tg < pt.gamma_no_carry_after_dense) sweep = false;
            if (sweep) mode = kPassSweep;
            // a bound pass that left most pairs candidates (the parameters jumped): back to the dense kernel
            if (mode == kPassBound && f.prune != 2 && known && L.mode == kPassBound && L.eval > pt.dense_again_above() * pairs_l) {
                mode = kPassDense;
                p.fell_back = true;
                p.bound_fail_act = L.act / pairs_l;
            }
        }
    }
    if (f.forget) p.bound_fail_act = -1.0;        // (a new restart: nothing is known about its bounds)
    // The cache of single-component rows (and the settled rows among them) survives every pruned pass over the same rows
    // whose M-step applied the delta lists - all of them end in rec_finish_kernel - including the one that regroups the
    // rows (regroup_rows moves the per-row state along).  A dense pass, new data or parameters unrelated to the last pass
    // drop it; rows that were settled then have no active pair on record, which only a pass that rebuilds everything
    // (bound or dense) can digest.
    // The rows are regrouped by dominant component at a bound pass (which rebuilds everything row-indexed anyway).  With
    // the proof round bound passes have become rare: the first time the responsibilities are sparse enough for the grouping
    // to pay (at most 2.5 active components per row) a carried pass therefore gives way to a bound pass, once - list-driven
    // kernels over ungrouped rows are 15-40 % slower for the rest of the fit.
    if (mode == kPassSweep && f.sort_rows && f.has_xp && !f.sorted && f.sorts == 0 && f.same_rows && f.after_estep && known &&
        L.act <= pt.regroup_force_below * rows_l && f.xc_of_x)
        mode = kPassBound;
    if (f.has_lock) {
        // (a regrouping of the rows takes the per-row state along: regroup_rows)
        const bool keep = mode != kPassDense && f.same_rows && !f.lock_reset && !f.delta_pending;
        if (f.lock_reset || (f.lock_live && !keep)) {
            if (mode == kPassSweep) mode = kPassBound;
            p.reset_cache = true;
        }
        p.settle = mode != kPassDense && f.cache_on && f.sparse && f.has_masks && f.has_xc && f.xc_of_x;
    }
    // a bound pass rebuilds everything row-indexed anyway: the moment to regroup the internal row order by the best
    // component of the previous pass (once at most 4 components per row are active: later passes are list-driven)
    p.regroup = mode == kPassBound && f.sort_rows && f.has_xp && !f.hmm && f.same_rows && f.after_estep && known &&
                L.act <= pt.regroup_below * rows_l && f.xc_of_x &&
                (!f.sorted || f.moved_since_sort > pt.regroup_moved * rows_l);      // (again once that share of the rows has moved on)
    // Rows with a single active component are settled (left out of the E-step as well as of the M-step) in every pruned
    // pass, provided the proof round is available - the int8 digit planes of this matrix are in the workspace, about the
    // pivot the component images were packed for: a settled row whose carried bounds no longer prove it then costs a few
    // int8 pairs.  (Without it such a row costs exact evaluations, and settling while the components still move by per
    // cents made rows come loose in masses - round 2 needed a gate with hysteresis on the drift, profiles/r2_experiments.md.)
    p.proof_capable = p.settle && f.opt_proof && f.xq_of_x && f.has_bound_images && f.xq_current;
    p.skip_margin = (p.proof_capable && f.settle_margin >= 0.0) ? f.settle_margin : -1.0;
    p.mode = mode;
    return p;
}

// Output blocks the int8 bound pass evaluates (fewer blocks: cheaper pass, looser bound, more candidates for the exact
// pass).  cand[l] = candidates per pair the last pass at level l left, act[l] = active pairs per pair when it was observed,
// seen[l] = pruned E-steps since (levels not seen for 32 passes count as unknown).
struct BoundLevel {
    int tb = 0;
    double cand[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};
    double act[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int seen[5] = {0, 0, 0, 0, 0};

    // `bound_images`: the workspace has the bound pass's 3-digit images; `carried_after`: the caller hands over drift hints (a
    // row-tiled pass, whose bounds do not survive the other tiles, does not) and one is pending; `wants_drift`: it would.
    void choose(int mode, bool bound_images, const gmmvb_pass_counters& L, bool known, bool carried_after, bool wants_drift,
                const PolicyTable& pt, int T, int D, int K) {
        if (mode == kPassBound && bound_images) {
            // How many output blocks the bound pass evaluates.  Cost model per (sample, component) pair, in units of
            // 1e-11 s (policy.h): bound pass i8_block_pair per block pair + i8_row_of_y per row of y; exact pass
            // f64_tile_pair per f64 tile pair of every candidate.  Take the cheapest level among those observed in the last 32
            // bound passes; look one level down when the current one leaves hardly any spare candidates or one level up
            // when more than half of its candidates are spare, if that level is unknown.
            // When the bounds are going to be carried (sweeps follow for tens of passes), all blocks: every nat of slack a bound
            // starts with postpones the pass in which it erodes into a candidate - measured at the benchmark shape (round 3):
            // four blocks instead of the model's three cost 6 ms once and take the following twenty passes from 8.1 to 7.2 ms
            // each (proof pairs halved, a quarter instead of 43 % of the sweep's columns opened).
            const int t32 = (D + 31) / 32;
            if (tb == 0) tb = t32 > 3 ? 3 : t32;
            if (carried_after) {
                tb = t32;
            } else if (known && L.mode == kPassBound) {
                const double pairs_l = L.rows * K;
                const int cur = tb;
                cand[cur] = L.eval / pairs_l;
                act[cur] = L.act / pairs_l;
                seen[cur] = 0;
                for (int l = 1; l <= t32; ++l)
                    if (l != cur && (++seen[l] > 32 || act[l] > 1.5 * act[cur] || act[l] < act[cur] / 1.5)) cand[l] = -1.0;
                const double gpp = pt.f64_tile_pair * tri_pairs(T);
                // carried passes follow a bound pass and inherit its spare candidates: a tighter bound pays for part of itself
                const double heirs = wants_drift ? 3.0 : 0.0;
                auto cost = [&](int l) {
                    const double spare_l = cand[l] > act[l] ? cand[l] - act[l] : 0.0;
                    return pt.i8_block_pair * tri_pairs(l) + pt.i8_row_of_y * 32 * l + gpp * (cand[l] + heirs * spare_l);
                };
                int best = cur;
                for (int l = 1; l <= t32; ++l)
                    if (cand[l] >= 0.0 && cost(l) < cost(best)) best = l;
                const double spare = cand[cur] - act[cur];
                if (best == cur) {
                    if (cur > 1 && cand[cur - 1] < 0.0 && spare * K < (heirs > 0.0 ? 0.02 : 0.25))
                        best = cur - 1;
                    else if (cur < t32 && cand[cur + 1] < 0.0 &&
                             spare * gpp > pt.i8_block_pair * (tri_pairs(cur + 1) - tri_pairs(cur)) + pt.i8_row_of_y * 32)
                        best = cur + 1;
                }
                tb = best;
            }
        }
        if (mode == kPassDense)      // whatever was learnt about the bound levels belongs to another regime
            for (double& c : cand) c = -1.0;
    }
};

}  // namespace gmmvb
