// Drives mstep_needs_counters and plan_mstep (bayesml_amd/csrc/mstep_plan.h) from a plain host compiler:
// tests/test_mstep_plan.py builds this file with -fsanitize=address,undefined, feeds it one case per line on stdin and
// compares what it prints.
//
//   key=value ...     overrides of a default MstepFacts -> needs_counters and the MstepPlan as key=value, then " | " and the
//                     refusal's message
//
// A value is a product of numbers and of the names n_rows, K and list_m_below (the values in force when they are met).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../bayesml_amd/csrc/mstep_plan.h"

using namespace gmmvb;

namespace {

double name(const MstepFacts& f, const std::string& n) {
    if (n == "n_rows") return (double)f.n_rows;
    if (n == "K") return f.K;
    if (n == "list_m_below") return f.list_m_below;
    char* end = nullptr;
    const double v = std::strtod(n.c_str(), &end);
    if (end == n.c_str() || *end != '\0') {
        std::fprintf(stderr, "unknown name '%s'\n", n.c_str());
        std::exit(2);
    }
    return v;
}

double value(const MstepFacts& f, const std::string& expr) {
    double prod = 1.0;
    std::stringstream factors(expr);
    for (std::string fac; std::getline(factors, fac, '*');) prod *= name(f, fac);
    return prod;
}

void set(MstepFacts& f, const std::string& key, double v) {
    const bool b = v != 0.0;
    if (key == "e_state") f.e_state = (int)v;
    else if (key == "e_rows") f.e_rows = (int64_t)v;
    else if (key == "n_rows") f.n_rows = (int64_t)v;
    else if (key == "ldx") f.ldx = (int64_t)v;
    else if (key == "K") f.K = (int)v;
    else if (key == "D") f.D = (int)v;
    else if (key == "T") f.T = (int)v;
    else if (key == "f64") f.x_dtype = b ? GMMVB_F64 : GMMVB_F32;
    else if (key == "vec") f.vec = b;
    else if (key == "generic") f.generic = b;
    else if (key == "wide") f.wide = b;
    else if (key == "has_xc") f.has_xc = b;
    else if (key == "xc_of_x") f.xc_of_x = b;
    else if (key == "xc_stale") f.xc_stale = b;
    else if (key == "sorted") f.sorted = b;
    else if (key == "has_xp") f.has_xp = b;
    else if (key == "sparse") f.sparse = b;
    else if (key == "has_masks") f.has_masks = b;
    else if (key == "act_rows") f.act_rows = (int64_t)v;
    else if (key == "rec_live") f.rec_live = b;
    else if (key == "lock_live") f.lock_live = b;
    else if (key == "delta_pending") f.delta_pending = b;
    else if (key == "mlists_done") f.mlists_done = b;
    else if (key == "mlists_lost") f.mlists_lost = b;
    else if (key == "active_lists") f.active_lists = b;
    else if (key == "S_cap") f.S_cap = (int)v;
    else if (key == "split_rows") f.split_rows = (int64_t)v;
    else if (key == "gen_S") f.gen_S = (int)v;
    else if (key == "kpw_pre") f.kpw_pre = (int)v;
    else if (key == "kpw_raw") f.kpw_raw = (int)v;
    else if (key == "lse_stale") f.lse_stale = b;
    else if (key == "hmm_no_lnrho") f.hmm_no_lnrho = b;
    else if (key == "hmm_skip_h") f.hmm_skip_h = b;
    else if (key == "opt_hmm_mstep_dense") f.opt_hmm_mstep_dense = b;
    else if (key == "opt_mlist_xc") f.opt_mlist_xc = b;
    else if (key == "lag_valid") f.lag_valid = b;
    else if (key == "lag_act") f.lag_act = v;
    else if (key == "list_m_below") f.list_m_below = v;
    else {
        std::fprintf(stderr, "unknown key '%s'\n", key.c_str());
        std::exit(2);
    }
}

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream words(line);
        MstepFacts f;
        bool any = false;
        for (std::string w; words >> w;) {
            if (w[0] == '#') break;
            const size_t eq = w.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "not key=value: '%s'\n", w.c_str());
                return 2;
            }
            set(f, w.substr(0, eq), value(f, w.substr(eq + 1)));
            any = true;
        }
        if (!any) continue;
        const MstepPlan p = plan_mstep(f);
        std::printf("needs_counters=%d status=%d kind=%d pre=%d need_prepare=%d need_row_lse=%d need_gamma_cm=%d need_recenter=%d "
                    "direct_r=%d gamma_weights=%d aux_lnrho=%d S=%lld rows_per_split=%lld grid=%lld KG=%d KGW=%d hmm_sparse_walk=%d "
                    "cap_chunks=%d r_min=%d lgrid=%lld dgrid=%lld rows=%d list_ldx=%lld apply_delta=%d build=%d qpart=%d "
                    "delta_pending=%d mlists_done=%d active_lists=%d clear_blk_fresh=%d reduce=%d add_cache=%d elems=%d "
                    "may_calibrate=%d counter=%d | %s\n",
                    (int)mstep_needs_counters(f), p.status, p.kind, (int)p.pre, (int)p.need_prepare, (int)p.need_row_lse,
                    (int)p.need_gamma_cm, (int)p.need_recenter, p.direct_r, (int)p.gamma_weights, (int)p.aux_lnrho, (long long)p.S,
                    (long long)p.rows_per_split, (long long)p.grid, p.KG, p.KGW, (int)p.hmm_sparse_walk, p.cap_chunks, p.r_min,
                    (long long)p.lgrid, (long long)p.dgrid, p.rows, (long long)p.list_ldx, (int)p.apply_delta, p.build, (int)p.qpart,
                    (int)p.delta_pending, (int)p.mlists_done, (int)p.active_lists, (int)p.clear_blk_fresh, p.reduce,
                    (int)p.add_cache, p.elems, (int)p.may_calibrate, p.counter, p.message);
    }
    return 0;
}
