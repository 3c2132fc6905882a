// Drives choose_pass and BoundLevel::choose (bayesml_amd/csrc/pass_plan.h) from a plain host compiler: tests/test_pass_plan.py
// builds this file with -fsanitize=address,undefined, feeds it one case per line on stdin and compares what it prints.
//
//   plan  key=value ...     overrides of a default PassFacts             -> the PassPlan as key=value
//   level key=value ...     a BoundLevel's state and choose()'s arguments -> the level's state afterwards
//
// A value is a sum of products of numbers and names: P (rows x K), rows, L.act, and the policy table's thresholds after
// init(8, 4) - the cases take their thresholds from the table, not from literals.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../bayesml_amd/csrc/pass_plan.h"

using namespace gmmvb;

namespace {

constexpr double kRows = 200000.0;

struct Case {
    PolicyTable pt;
    PassFacts f;
    BoundLevel level;
    std::map<std::string, double> extra;      // choose()'s arguments that are no facts

    double name(const std::string& n) const {
        if (n == "P") return kRows * f.K;
        if (n == "rows") return kRows;
        if (n == "L.act") return f.L.act;
        if (n == "prune_below") return pt.prune_below();
        if (n == "dense_again_above") return pt.dense_again_above();
        if (n == "regroup_force_below") return pt.regroup_force_below;
        if (n == "regroup_below") return pt.regroup_below;
        if (n == "regroup_moved") return pt.regroup_moved;
        if (n == "overflow_rows") return pt.overflow_rows;
        if (n == "carried_eval_above") return pt.carried_eval_above;
        if (n == "sweep_after_dense_below") return pt.sweep_after_dense_below;
        if (n == "gamma_no_carry") return pt.gamma_no_carry;
        if (n == "gamma_no_carry_after_dense") return pt.gamma_no_carry_after_dense;
        if (n == "dense") return kPassDense;
        if (n == "bound") return kPassBound;
        if (n == "sweep") return kPassSweep;
        char* end = nullptr;
        const double v = std::strtod(n.c_str(), &end);
        if (end == n.c_str() || *end != '\0') {
            std::fprintf(stderr, "unknown name '%s'\n", n.c_str());
            std::exit(2);
        }
        return v;
    }
    double value(const std::string& expr) const {
        double sum = 0.0;
        std::stringstream terms(expr);
        for (std::string term; std::getline(terms, term, '+');) {
            double prod = 1.0;
            std::stringstream factors(term);
            for (std::string fac; std::getline(factors, fac, '*');) prod *= name(fac);
            sum += prod;
        }
        return sum;
    }
    void set(const std::string& key, double v) {
        const bool b = v != 0.0;
        gmmvb_pass_counters& L = f.L;
        if (key == "L.valid") L.valid = b;
        else if (key == "L.act") L.act = v;
        else if (key == "L.eval") L.eval = v;
        else if (key == "L.over") L.over = v;
        else if (key == "L.settled") L.settled = v;
        else if (key == "L.listed") L.listed = v;
        else if (key == "L.proof") L.proof = v;
        else if (key == "L.rows") L.rows = v;
        else if (key == "L.mode") L.mode = (int)v;
        else if (key == "known") f.known = b;
        else if (key == "can_prune") f.can_prune = b;
        else if (key == "big") f.big = b;
        else if (key == "prune") f.prune = (int)v;
        else if (key == "forget") f.forget = b;
        else if (key == "same_rows") f.same_rows = b;
        else if (key == "after_estep") f.after_estep = b;
        else if (key == "prev_lists") f.prev_lists = b;
        else if (key == "have_drift") f.have_drift = b;
        else if (key == "opt_carry_off") f.opt_carry_off = b;
        else if (key == "dense_valid") f.dense_valid = b;
        else if (key == "can_project") f.can_project = b;
        else if (key == "opt_project") f.opt_project = (int)v;
        else if (key == "typical_gamma") f.typical_gamma = v;
        else if (key == "bound_fail_act") f.bound_fail_act = v;
        else if (key == "bound_tb") f.bound_tb = (int)v;
        else if (key == "T") f.T = (int)v;
        else if (key == "K") f.K = (int)v;
        else if (key == "D") f.D = (int)v;
        else if (key == "n_rows") f.n_rows = (int64_t)v;
        else if (key == "sort_rows") f.sort_rows = b;
        else if (key == "has_xp") f.has_xp = b;
        else if (key == "sorted") f.sorted = b;
        else if (key == "sorts") f.sorts = (int64_t)v;
        else if (key == "moved_since_sort") f.moved_since_sort = v;
        else if (key == "has_xc") f.has_xc = b;
        else if (key == "xc_of_x") f.xc_of_x = b;
        else if (key == "hmm") f.hmm = b;
        else if (key == "has_lock") f.has_lock = b;
        else if (key == "lock_reset") f.lock_reset = b;
        else if (key == "lock_live") f.lock_live = b;
        else if (key == "delta_pending") f.delta_pending = b;
        else if (key == "cache_on") f.cache_on = b;
        else if (key == "sparse") f.sparse = b;
        else if (key == "has_masks") f.has_masks = b;
        else if (key == "opt_proof") f.opt_proof = b;
        else if (key == "xq_of_x") f.xq_of_x = b;
        else if (key == "has_bound_images") f.has_bound_images = b;
        else if (key == "xq_current") f.xq_current = b;
        else if (key == "settle_margin") f.settle_margin = v;
        else if (key == "tb") level.tb = (int)v;
        else if (key.size() == 5 && key.compare(0, 4, "cand") == 0 && key[4] >= '0' && key[4] <= '4') level.cand[key[4] - '0'] = v;
        else if (key.size() == 4 && key.compare(0, 3, "act") == 0 && key[3] >= '0' && key[3] <= '4') level.act[key[3] - '0'] = v;
        else if (key.size() == 5 && key.compare(0, 4, "seen") == 0 && key[4] >= '0' && key[4] <= '4') level.seen[key[4] - '0'] = (int)v;
        else if (key == "mode" || key == "carried_after" || key == "wants_drift") extra[key] = v;
        else {
            std::fprintf(stderr, "unknown key '%s'\n", key.c_str());
            std::exit(2);
        }
    }
};

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream words(line);
        std::string kind;
        if (!(words >> kind) || kind[0] == '#') continue;
        Case c;
        c.pt.init(8, 4);
        c.f.K = 64;      // (names that depend on K read the value in force when they are met)
        for (std::string w; words >> w;) {
            const size_t eq = w.find('=');
            if (eq == std::string::npos) {
                std::fprintf(stderr, "not key=value: '%s'\n", w.c_str());
                return 2;
            }
            c.set(w.substr(0, eq), c.value(w.substr(eq + 1)));
        }
        if (kind == "plan") {
            const PassPlan p = choose_pass(c.pt, c.f);
            std::printf("mode=%d fell_back=%d bound_fail_act=%.6g spare_set=%d regroup=%d reset_cache=%d settle=%d proof_capable=%d "
                        "skip_margin=%.6g\n", p.mode, (int)p.fell_back, p.bound_fail_act, (int)p.spare_set, (int)p.regroup,
                        (int)p.reset_cache, (int)p.settle, (int)p.proof_capable, p.skip_margin);
        } else if (kind == "level") {
            c.level.choose((int)c.extra["mode"], c.f.has_bound_images, c.f.L, c.f.known, c.extra["carried_after"] != 0.0,
                           c.extra["wants_drift"] != 0.0, c.pt, c.f.T, c.f.D, c.f.K);
            std::printf("tb=%d", c.level.tb);
            for (int l = 1; l <= 4; ++l) std::printf(" cand%d=%.6g act%d=%.6g seen%d=%d", l, c.level.cand[l], l, c.level.act[l], l, c.level.seen[l]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown kind '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
