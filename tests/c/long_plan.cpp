// long_plan.cpp -- the plan of a batch's reads beyond 2048 events, plan_long_reads (sfa_plan.hpp), without a GPU
// (tests/test_long_plan_cpu.py).  Prints the geometry constants ("consts ...") and one line per plan: "plan <name>", the inputs,
// then every field of the LongPlan and, per group, begin:size:set:off_word:strips.  The expected values are stated by the test.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "sfa_plan.hpp"

template <typename T>
static std::string join(const std::vector<T> &v) {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return v.empty() ? "-" : s;
}

struct Case {
    const char *name;
    std::vector<int32_t> jobs;
    std::vector<int32_t> qlens;  // the whole batch, short reads included
    int64_t interval, budget, cu, spin;
};

static std::vector<int32_t> times(int n, int32_t qlen, std::vector<int32_t> then = {}) {
    std::vector<int32_t> v(n, qlen);
    v.insert(v.end(), then.begin(), then.end());
    return v;
}

static void print(const Case &k) {
    std::vector<int64_t> q_off(1, 0);
    for (int32_t l : k.qlens) q_off.push_back(q_off.back() + l);
    const sfa::LongPlan p = sfa::plan_long_reads(q_off.data(), static_cast<int32_t>(k.qlens.size()), k.jobs, k.interval, k.budget, k.cu, k.spin);
    printf("plan %s jobs=%s qlens=%s interval=%lld budget=%lld cu=%lld spin=%lld", k.name, join(k.jobs).c_str(), join(k.qlens).c_str(), (long long)k.interval,
           (long long)k.budget, (long long)k.cu, (long long)k.spin);
    printf(" n_long=%d reads=%s n_strips=%s events=%lld max=%lld max_strips=%d", p.n_long(), join(p.reads).c_str(), join(p.n_strips).c_str(), (long long)p.events,
           (long long)p.max, p.max_strips);
    printf(" bnd_off=%s cost_rows=%lld bnd_stride=%lld ck_shift=%d ck_off=%s", join(p.bnd_off).c_str(), (long long)p.cost_rows, (long long)p.bnd_stride, p.ck_shift,
           join(p.ck_off).c_str());
    printf(" group=%d n_groups=%d two_sets=%d strip_off=%s", p.group, p.n_groups, p.two_sets ? 1 : 0, join(p.strip_off).c_str());
    printf(" sg_reads=%zu sg_bnd=%zu sg_ck=%zu sg_soff=%zu sg_bytes=%zu", p.sg.reads, p.sg.bnd, p.sg.ck, p.sg.soff, p.sg.bytes);
    printf(" prog_bytes=%zu bndc_floats=%zu lck_floats=%zu n_part=%zu limit_ms=%lld groups=", p.prog_bytes, p.bndc_floats, p.lck_floats, p.n_part, (long long)p.limit_ms);
    for (int32_t gi = 0; gi < p.n_groups; ++gi) printf("%s%d:%d:%d:%d:%d", gi ? ";" : "", p.begin(gi), p.size(gi), p.set(gi), p.off_word(gi), p.strips_of(gi));
    printf("%s\n", p.n_groups ? "" : "-");
}

int main() {
    const std::vector<int32_t> ncov = {29898, 29898}, three = {100, 5000, 29898};  // (a job shorter than the query in `three`)
    const int64_t GiB = 1ll << 30, ample = 16 * GiB;
    // checkpoint bytes of two 5000-event reads on ncov at T = 512 / 1024 / 2048 (3 strips x 58 / 29 / 14 records x 2 jobs x 8448 bytes x 2 reads)
    const int64_t ck9 = 3 * 58 * 2 * 8448ll * 2, ck10 = 3 * 29 * 2 * 8448ll * 2, ck11 = 3 * 14 * 2 * 8448ll * 2;
    // one 5000-event read on ncov at T = 512: 2 boundary rows of 2 x 30156 words, 348 checkpoint records
    const int64_t read5000 = 2 * 2 * 30156 * 4ll + 348 * 8448ll;
    const std::vector<Case> cases = {
        {"one_2049", ncov, {2049}, 0, ample, 256, 20000},
        {"one_4096", ncov, {4096}, 0, ample, 256, 20000},
        {"one_4097", ncov, {4097}, 0, ample, 256, 20000},
        {"mixed", three, {250, 2049, 6500, 2048, 4097, 20000, 0, 4096}, 0, ample, 256, 20000},
        {"none", ncov, {250, 2048, 0}, 0, ample, 256, 20000},
        {"interval_4", ncov, {5000, 5000}, 4, 1, 256, 20000},
        {"interval_64", ncov, {5000, 5000}, 64, 1, 256, 20000},
        {"interval_512", ncov, {5000, 5000}, 512, 1, 256, 20000},
        {"budget_fits_9", ncov, {5000, 5000}, 0, ck9, 256, 20000},
        {"budget_below_9", ncov, {5000, 5000}, 0, ck9 - 1, 256, 20000},
        {"budget_fits_10", ncov, {5000, 5000}, 0, ck10, 256, 20000},
        {"budget_below_10", ncov, {5000, 5000}, 0, ck10 - 1, 256, 20000},
        {"budget_below_11", ncov, {5000, 5000}, 0, ck11 - 1, 256, 20000},
        {"budget_one_byte", ncov, {5000, 5000}, 0, 1, 256, 20000},
        {"groups_1mib", ncov, {2500, 5000, 2049}, 0, 1 << 20, 256, 20000},
        {"groups_16gib", ncov, {2500, 5000, 2049}, 0, ample, 256, 20000},
        {"waves_below_cu1", ncov, times(14, 4096, {4097}), 0, ample, 1, 20000},                // 31 strips x 2 jobs = 62 < 64
        {"waves_at_cu1", ncov, times(16, 4096), 0, ample, 1, 20000},                          // 32 strips x 2 jobs = 64
        {"waves_below_cu256", ncov, times(818, 20000, {4097, 4096, 4096, 4096, 4096}), 0, 1024 * GiB, 256, 20000},  // 8191 strips: 16382 < 16384
        {"waves_at_cu256", ncov, times(819, 20000, {4096}), 0, 1024 * GiB, 256, 20000},       // 8192 strips: 16384
        {"two_per_set", ncov, times(5, 5000), 512, 4 * read5000, 256, 20000},
        {"two_per_set_upper", ncov, times(5, 5000), 512, 6 * read5000 - 1, 256, 20000},
        {"limit_option", three, {20000}, 0, ample, 256, 20000},
        {"limit_floor", three, {20000}, 0, ample, 256, 1},
        {"limit_floor_short", three, {2049}, 0, ample, 256, 0},
    };
    printf("consts kStripR=%d kStripRows=%d kCkRec=%d kBndPad=%d kPipeBlock=%d kMaxQuery=%d\n", sfa::kStripR, sfa::kStripRows, sfa::kCkRec, sfa::kBndPad, sfa::kPipeBlock,
           sfa::kMaxQuery);
    for (const Case &k : cases) print(k);
    printf("done %zu\n", cases.size());
    return 0;
}
