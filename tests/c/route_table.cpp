// route_table.cpp -- the route sfa_plan.hpp picks for synthetic batches: plan_batch() + choose_route() (tests/test_route_table.py).
// stdin: one case per line, "name key=value ...", keys as in `o` below (n reads of qlen events each, jobs references of job_len
// columns, sims SIMDs); stdout: "name route" per case.
#include <cstdint>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "sfa_plan.hpp"

int main() {
    const char *names[] = {"NoQuads", "Segments", "Lds", "LdsFused", "Fused32", "Secondary", "TwoPass"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name, kv;
        in >> name;
        std::map<std::string, int64_t> o = {{"n", 64},  {"qlen", 100},   {"jobs", 1},  {"job_len", 10000}, {"sims", 8},     {"widening", 1},
                                            {"lds", 1}, {"fused", 1},    {"std", 0},   {"sec", 0},         {"segments", 0}, {"interval", 0}};
        while (in >> kv) o.at(kv.substr(0, kv.find('='))) = std::stoll(kv.substr(kv.find('=') + 1));
        std::vector<int64_t> q_off(o["n"] + 1, 0);
        for (int64_t i = 0; i < o["n"]; ++i) q_off[i + 1] = q_off[i] + o["qlen"];
        const std::vector<int32_t> job_len(o["jobs"], static_cast<int32_t>(o["job_len"]));
        sfa::PlanParams pp;
        pp.n_sims = o["sims"];
        pp.lane_widening = o["widening"];
        pp.column_segments = o["segments"];
        pp.ckpt_interval = o["interval"];
        pp.std_dtw = o["std"] != 0;
        pp.skip_long = o["qlen"] > sfa::kMaxQuery;
        // the planner inputs the library derives from its options (sfa_align.hip, plan_params)
        pp.allow_segments = !pp.std_dtw && o["sec"] == 0;
        pp.lds_ckpt = o["sec"] > 0 ? 0 : static_cast<int>(o["lds"]);
        sfa::BatchPlan plan;
        std::string err;
        if (sfa::plan_batch(q_off.data(), static_cast<int32_t>(o["n"]), job_len, o["jobs"] * o["job_len"], pp, &plan, &err)) {
            std::cout << name << " error:" << err << "\n";
            continue;
        }
        // wave slots: SIMDs * SFA_LCK_WAVES (4, sdtw_kernels.hpp)
        const sfa::Route r = sfa::choose_route(plan, pp.std_dtw, static_cast<int>(o["sec"]), o["fused"], o["sims"] * 4);
        std::cout << name << " " << names[static_cast<int>(r)] << "\n";
    }
    return 0;
}
