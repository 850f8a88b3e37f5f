// The planner (sigfish_amd/csrc/sfa_plan.hpp: plan_batch over chunks_for, split_jobs, the column segments) as a stand-alone host
// program, for tests/test_tie_cases_cpu.py: where the job list of a batch is cut, so that a tie a case claims to lie across a
// chunk boundary can be shown to lie across one.  It reads requests from stdin:
//   plan <n_sims> <lane_widening> <column_segments> <secondary> <std_dtw> <n_reads> <n_jobs>, then the n_reads query lengths and
//   the n_jobs job lengths (a job is one strand array of one contig, in processing order)
//     -> "plan <widening> <n_quads> <n_chunks> <n_seg> <warm_windows> <max_lanes> <chunk_begin x (n_chunks + 1)>"
// with the other parameters at the context's defaults and set as sfa_align.hip sets them (no column segments for --dtw-std or with
// secondary mappings; reads beyond kMaxQuery events leave the wave kernels for the row strips).
#include <cstdio>
#include <cstring>

#include "sfa_plan.hpp"

int main() {
    char word[16];
    int n_plans = 0;
    while (scanf("%15s", word) == 1) {
        if (strcmp(word, "plan") != 0) return 2;
        long long n_sims = 0, widening = 0, segments = 0;
        int secondary = 0, std_dtw = 0, n = 0, n_jobs = 0;
        if (scanf("%lld %lld %lld %d %d %d %d", &n_sims, &widening, &segments, &secondary, &std_dtw, &n, &n_jobs) != 7 || n < 0 || n_jobs < 1) return 3;
        std::vector<int64_t> q_off(n + 1, 0);
        bool any_long = false;
        for (int i = 0; i < n; ++i) {
            long long l = 0;
            if (scanf("%lld", &l) != 1 || l < 0) return 4;
            q_off[i + 1] = q_off[i] + l;
            any_long = any_long || l > sfa::kMaxQuery;
        }
        std::vector<int32_t> job_len(n_jobs);
        int64_t total = 0;
        for (int j = 0; j < n_jobs; ++j) {
            if (scanf("%d", &job_len[j]) != 1 || job_len[j] < 1) return 5;
            total += job_len[j];
        }
        sfa::PlanParams pp;
        pp.n_sims = n_sims;
        pp.lane_widening = widening;
        pp.column_segments = segments;
        pp.std_dtw = std_dtw != 0;
        pp.allow_segments = !pp.std_dtw && secondary == 0;
        pp.lds_ckpt = secondary > 0 ? 0 : 1;
        pp.skip_long = any_long;
        sfa::BatchPlan p;
        std::string err;
        if (sfa::plan_batch(q_off.data(), n, job_len, total, pp, &p, &err) != 0) {
            printf("FAIL %s\n", err.c_str());
            return 6;
        }
        if (static_cast<int>(p.chunk_begin.size()) != p.n_chunks + 1) return 7;
        printf("plan %d %d %d %d %d %d", p.widening, p.n_quads, p.n_chunks, p.n_seg, p.warm_windows, p.max_lanes);
        for (int32_t b : p.chunk_begin) printf(" %d", b);
        printf("\n");
        ++n_plans;
    }
    printf("done %d\n", n_plans);
    return 0;
}
