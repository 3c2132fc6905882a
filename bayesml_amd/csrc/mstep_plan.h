// Which form the M-step takes (generic, dense MFMA, one-tile small, HMM small, wide, or per-component lists), its launch
// geometry, the rows the list kernel reads, and what becomes of the settled-row cache's flags - or why the call is refused.
//
// Plain C++: gmmvb_mstep (capi_mstep.hip) fills MstepFacts from the workspace, fetches the E-step's counters when
// mstep_needs_counters says the answer depends on them, calls plan_mstep and carries the plan out;
// tests/mstep_plan_cases.cpp drives the same two functions from a host compiler.  No HIP header here.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "tri_index.h"
#include "workspace_plan.h"      // round_up, the status codes and dtypes of include/gmmvb.h

namespace gmmvb {

// list entries per chunk of the list M-step (2048: +4 %, 4096: +19 % on the list M-step, round 2)
#ifndef GMMVB_MLIST_RMIN
#define GMMVB_MLIST_RMIN 1024
#endif
constexpr int kMlistRmin = GMMVB_MLIST_RMIN;
constexpr int kMstepSmallCw = 8;      // one feature tile: a wave walks the rows once for eight components (mstep.h, mstep_small_f64)

enum MstepKind { kMstepGeneric = 0, kMstepMfma = 1, kMstepSmall = 2, kMstepHmmSmall = 3, kMstepWide = 4, kMstepLists = 5 };
enum MstepRows { kRowsCentred = 0, kRowsXp32 = 1, kRowsX32 = 2 };      // list kernel: the centred f64 copy, xp as f32, the caller's f32 rows
enum MstepBuild { kBuildNone = 0, kBuildMmask = 1, kBuildMasks = 2 };  // lists from mmask / mblk (rows in the cache left out), or masks / blk
enum MstepReduce { kReduceGeneric = 0, kReduceStats = 1, kReduceChunks = 2 };

// Everything the decision reads, as values.
struct MstepFacts {
    // state
    int e_state = 0;
    int64_t e_rows = 0, n_rows = 0, ldx = 0;
    int K = 0, D = 0, T = 0, x_dtype = GMMVB_F64;
    bool vec = false;                // check_x: the caller's rows can be read with vector loads
    // shape
    bool generic = false, wide = false, has_xc = false, xc_of_x = false, xc_stale = false, sorted = false, has_xp = false;
    // lists and the cache of settled rows
    bool sparse = false, has_masks = false;
    int64_t act_rows = 0;
    bool rec_live = false, lock_live = false, delta_pending = false, mlists_done = false, mlists_lost = false,
         active_lists = false;
    // geometry
    int S_cap = 0;
    int64_t split_rows = 0;
    int gen_S = 1;
    int kpw_pre = 1, kpw_raw = 1;    // mstep_components_per_wg(T, pre) for pre true / false
    // HMM
    bool lse_stale = false, hmm_no_lnrho = false, hmm_skip_h = false, opt_hmm_mstep_dense = false;
    bool opt_mlist_xc = false;       // GMMVB_MLIST_XC=1: the list kernel always reads the centred f64 copy
    // policy: the counters of the E-step (ws->lag, after fetch_counters where mstep_needs_counters asked for it)
    bool lag_valid = false;
    double lag_act = 0.0;
    double list_m_below = 0.0;       // PolicyTable::list_m_below()
};

// Everything the decision produces.  A refused call (status != GMMVB_OK) keeps the steps the M-step takes before it finds
// out: the flags set in the plan are carried out, then `message` is returned.  For every refusal but the last one (the
// lists were lost to a read-out, kind == kMstepLists) that is before anything of the pass itself is launched.
struct MstepPlan {
    int status = GMMVB_OK;
    const char* message = "";
    int kind = kMstepMfma;
    bool pre = false;                // the kernel reads the centred copy
    bool need_prepare = false;       // wide rows nobody prepared: gmmvb_prepare_rows first
    bool need_row_lse = false;       // a mixture M-step on an HMM workspace: the rows' log-normalisers after all
    bool need_gamma_cm = false;      // the component-major copy of gamma (hmm_ensure_gamma_cm)
    bool need_recenter = false;      // the centred copy is read and is not in the internal row order
    int direct_r = 0;                // 0: r = exp(ln rho - lse), 1: loaded responsibilities, 2: HMM gamma
    bool gamma_weights = false;      // the weights are gamma (component-major, or time-major for kMstepHmmSmall), not the ln rho array
    bool aux_lnrho = false;          // h = sum gamma ln rho: the ln rho array goes in as `aux`
    // dense geometry (generic: S and rows_per_split only)
    int64_t S = 0, rows_per_split = 0, grid = 0;
    int KG = 0;                      // component groups of a workgroup row
    int KGW = 0;                     // ... of the one-tile kernels (4 waves of kMstepSmallCw components)
    bool hmm_sparse_walk = false;    // kMstepHmmSmall: only the MFMA steps with a gamma above the relevance line are walked
    // lists
    int cap_chunks = 0, r_min = 0;
    int64_t lgrid = 0, dgrid = 0;
    int rows = kRowsCentred;
    int64_t list_ldx = 0;            // row stride of an f32 source
    bool apply_delta = false;        // the delta lists of the cache go first
    int build = kBuildNone;
    bool qpart = false;              // builders of delta and mmask lists get the per-block pair counts (masks: never)
    bool delta_pending = false, mlists_done = false, active_lists = false;      // the workspace's flags afterwards
    bool clear_blk_fresh = false;
    int reduce = kReduceStats;
    bool add_cache = false;          // reduce_chunks adds the cache of settled rows
    int elems = 0;                   // doubles of one component's statistics in a slab (non-generic)
    bool may_calibrate = false;      // a dense MFMA pass over E-step output: the policy table may time it (cal_wanted)
    int counter = 5;                 // gmmvb_pass_counts slot: 5 dense, 6 lists

    MstepPlan& refuse(const char* why) {
        status = GMMVB_ESTATE;
        message = why;
        return *this;
    }
};

namespace mstep_detail {
inline bool has_responsibilities(const MstepFacts& f) { return !(f.e_state == 0 || f.e_state == 4 || f.e_rows != f.n_rows); }
// (past 8 feature tiles the M-step only exists over the centred copy: it is made by the call if the caller has not)
inline bool auto_prepare(const MstepFacts& f) { return f.wide && f.has_xc && !f.xc_of_x; }
inline bool pre(const MstepFacts& f) { return f.has_xc && (f.xc_of_x || f.wide); }
// E-step output whose active pairs were counted, over the matrix of the E-step
inline bool list_eligible(const MstepFacts& f) {
    return f.sparse && f.has_masks && pre(f) && f.e_state == 1 && f.act_rows == f.n_rows;
}
}  // namespace mstep_detail

// After a dense E-step the lists pay off below a share of active pairs: the host has been waiting for that kernel anyway
// and reads this pass's own count - a blocking fetch, asked for only where the answer depends on it.
inline bool mstep_needs_counters(const MstepFacts& f) {
    using namespace mstep_detail;
    if (!has_responsibilities(f) || f.generic) return false;
    if (!pre(f) && f.sorted) return false;      // (refused before the counters are looked at)
    return list_eligible(f) && !f.rec_live;
}

// The list form: only the samples that can change the f64 sums, through per-component lists cut into chunks (mstep.h) - as
// many slabs as the workspace holds, at least r_min entries per chunk; kpw: components per workgroup over the centred copy.
// `p` comes with the workspace's three list flags as they are.
inline MstepPlan plan_mstep_lists(const MstepFacts& f, int kpw, MstepPlan p) {
    p.kind = kMstepLists;
    p.counter = 6;
    p.cap_chunks = (int)std::min<int64_t>((int64_t)f.S_cap * f.K, 1 << 30);
    p.r_min = kMlistRmin;
    // f32 rows with whole 16-feature tiles: read them instead of the twice as wide centred copy
    if (!f.opt_mlist_xc && f.x_dtype == GMMVB_F32 && f.D == 16 * f.T && (f.T == 2 || f.T == 4 || f.T == 8)) {
        if (f.sorted) {
            if (f.has_xp) p.rows = kRowsXp32, p.list_ldx = f.D;
        } else if (f.vec) {
            p.rows = kRowsX32, p.list_ldx = f.ldx;
        }
    }
    p.need_recenter = p.rows == kRowsCentred && f.xc_stale;
    p.lgrid = (p.cap_chunks + kpw - 1) / kpw;
    const int64_t most = (f.n_rows * (int64_t)f.K + p.r_min - 1) / p.r_min + f.K;      // no more chunks than this can exist
    p.lgrid = std::min(p.lgrid, (most + kpw - 1) / kpw);
    p.qpart = f.e_state == 1;
    if (f.lock_live && f.delta_pending) {
        // the rows that settled or came loose in this pass (rec_finish_kernel's delta masks) enter / leave the cache of
        // settled rows - before the pass's own lists are built in the same buffers.  At most one entry per row: far fewer
        // chunks than the lists of a pass can have
        p.apply_delta = true;
        p.dgrid = std::min(((f.n_rows + p.r_min - 1) / p.r_min + f.K + kpw - 1) / kpw, p.lgrid);
        p.delta_pending = p.active_lists = p.mlists_done = false;
    }
    // masks and block counts of the active pairs were written by lse_mask_kernel / rec_finish_kernel at the end of the E-step
    if (f.lock_live) {
        // the rows in the cache are left out: the M-step has its own masks (the E-step's next first round builds its lists
        // from the full ones)
        if (!p.mlists_done) {
            if (f.mlists_lost)
                return p.refuse("the M-step's lists were used by a read-out of settled rows: call gmmvb_estep again");
            p.build = kBuildMmask;
            p.mlists_done = true;
            p.active_lists = false;
        }
    } else if (!p.active_lists) {
        p.build = kBuildMasks;
        p.active_lists = true;
        p.clear_blk_fresh = true;
    }
    p.grid = p.lgrid;
    p.S = 0;
    p.rows_per_split = p.r_min;
    p.reduce = kReduceChunks;
    p.add_cache = f.lock_live;
    return p;
}

inline MstepPlan plan_mstep(const MstepFacts& facts) {
    using namespace mstep_detail;
    MstepFacts f = facts;            // (the steps of the plan change some of them on the way)
    MstepPlan p;
    if (!has_responsibilities(f))
        return p.refuse("no responsibilities for these rows: call gmmvb_estep or gmmvb_load_responsibilities first");
    p.need_row_lse = f.lse_stale && f.e_state == 1;
    p.direct_r = f.e_state == 2 ? 1 : (f.e_state == 3 ? 2 : 0);
    p.gamma_weights = f.e_state == 3;
    p.delta_pending = f.delta_pending, p.mlists_done = f.mlists_done, p.active_lists = f.active_lists;
    if (f.generic) {
        p.kind = kMstepGeneric;
        p.need_gamma_cm = f.e_state == 3;
        p.aux_lnrho = f.e_state == 3 && !f.hmm_skip_h;
        p.rows_per_split = round_up((f.n_rows + f.gen_S - 1) / f.gen_S, 64);
        p.S = (f.n_rows + p.rows_per_split - 1) / p.rows_per_split;
        p.reduce = kReduceGeneric;
        return p;
    }
    p.elems = tri_pairs(f.T) * 256 + 16 * f.T + 2;
    // row splits: ~4 workgroups per CU in total, whole 64-row groups per split, S a multiple of 8 where possible
    p.S = std::min<int64_t>(f.S_cap, (f.n_rows + 63) / 64);
    p.rows_per_split = round_up((f.n_rows + p.S - 1) / p.S, 64);
    if (f.split_rows && p.rows_per_split > f.split_rows) p.rows_per_split = f.split_rows;
    p.S = (f.n_rows + p.rows_per_split - 1) / p.rows_per_split;
    p.pre = pre(f);
    if (auto_prepare(f)) {           // gmmvb_prepare_rows: the caller's row order, a fresh copy, no settled rows
        p.need_prepare = true;
        f.sorted = f.xc_stale = f.lock_live = false;
    }
    const int kpw = p.pre ? f.kpw_pre : f.kpw_raw;
    p.KG = (f.K + kpw - 1) / kpw;
    p.grid = 8 * ((p.S + 7) / 8) * p.KG;
    const bool hmm_small = f.e_state == 3 && f.T == 1 && p.pre;      // reads gamma time-major (hmm_mstep_small_kernel)
    if (f.e_state == 3) {            // HMM: responsibilities = gamma from the forward-backward pass, h = sum gamma ln rho
        p.need_gamma_cm = !hmm_small;
        p.aux_lnrho = !(f.hmm_no_lnrho || f.hmm_skip_h);      // (else h stays 0, see hmmvb_skip_h / hmmvb_emission_target)
    }
    if (!p.pre && f.sorted)
        return p.refuse("the workspace's rows are regrouped for another sample matrix: call gmmvb_prepare_rows first");
    // the lists pay off while act kListMns < K kDenseMns (list_m_below).  A pruned E-step leaves exact values for the listed
    // pairs only (the others are bounded in the f32 array, not in ln rho): its M-step always runs over the lists, however
    // many pairs are active
    bool lists = list_eligible(f);
    if (lists && !f.rec_live) lists = f.lag_valid && f.lag_act <= f.list_m_below * ((double)f.n_rows * f.K);
    if (lists && f.K > 256) lists = false;
    if (f.rec_live && f.e_state == 1 && !lists)
        return p.refuse("a pruned E-step needs the list M-step over the matrix of the E-step (gmmvb_prepare_rows)");
    if (f.lock_live && !lists)
        return p.refuse("settled rows need the list M-step over the matrix of the E-step (gmmvb_prepare_rows)");
    if (!lists) {
        p.need_recenter = p.pre && f.xc_stale;      // the dense kernel reads the centred copy in the internal row order
        if (f.T == 1 && p.pre) {
            p.kind = hmm_small ? kMstepHmmSmall : kMstepSmall;
            p.hmm_sparse_walk = hmm_small && !f.opt_hmm_mstep_dense;
            p.KGW = (f.K + 4 * kMstepSmallCw - 1) / (4 * kMstepSmallCw);
            p.grid = 8 * ((p.S + 7) / 8) * p.KGW;
        } else {
            p.kind = f.wide ? kMstepWide : kMstepMfma;
            p.may_calibrate = p.direct_r == 0;
        }
        return p;
    }
    return plan_mstep_lists(f, kpw, p);
}

}  // namespace gmmvb
