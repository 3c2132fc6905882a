// Host-side cases for the carried sweep's run length (bayesml_amd/csrc/workspace_plan.h: sweep_run_length,
// dispatch_sweep_run and the GMMVB_SWEEP_RUN switch of WorkspaceOptions::read).  One line per query on stdin:
//   length K asked             -> sweep_run_length(K, asked), then the constant dispatch_sweep_run hands out for it
//   option env.NAME=VALUE ...  -> opt_sweep_run of WorkspaceOptions::read over that environment
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../bayesml_amd/csrc/workspace_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "length") {
            int K = 0, asked = 0, handed = -1;
            in >> K >> asked;
            const int run = gmmvb::sweep_run_length(K, asked);
            gmmvb::dispatch_sweep_run(run, [&](auto rr) { handed = decltype(rr)::value; });
            std::cout << run << " " << handed << "\n";
        } else if (what == "option") {
            std::map<std::string, std::string> env;
            std::string kv;
            while (in >> kv) {
                const size_t eq = kv.find('=');
                if (kv.rfind("env.", 0) == 0 && eq != std::string::npos) env[kv.substr(4, eq - 4)] = kv.substr(eq + 1);
            }
            const gmmvb::WorkspaceOptions o = gmmvb::WorkspaceOptions::read([&env](const char* name) -> const char* {
                auto it = env.find(name);
                return it == env.end() ? nullptr : it->second.c_str();
            });
            std::cout << o.opt_sweep_run << "\n";
        } else {
            return 2;
        }
    }
    return 0;
}
