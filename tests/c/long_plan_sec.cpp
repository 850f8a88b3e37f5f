// long_plan_sec.cpp -- what plan_long_reads (sfa_plan.hpp) says about the secondaries of the long reads ("secondary_strips"):
// the words of the candidate lists and of the rank arrays, and where rank k of a long read lies, without a GPU
// (tests/test_secondary_strips_cpu.py).  Prints one line "sec <name> ..." per plan with the fields, checks the layout itself
// ("FAIL ..." lines) and ends with "done <failures>".
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "sfa_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            ++failures;               \
            printf("FAIL " __VA_ARGS__); \
            printf("\n");             \
        }                             \
    } while (0)

struct Case {
    const char *name;
    std::vector<int32_t> jobs, qlens;
    int64_t interval, budget;
};

static void run(const Case &k) {
    std::vector<int64_t> q_off(1, 0);
    for (int32_t l : k.qlens) q_off.push_back(q_off.back() + l);
    const sfa::LongPlan p = sfa::plan_long_reads(q_off.data(), static_cast<int32_t>(k.qlens.size()), k.jobs, k.interval, k.budget, 256, 20000);
    const size_t n_long = p.reads.size(), n_jobs = k.jobs.size();
    printf("sec %s n_long=%zu n_jobs=%zu n_part=%zu group=%d n_groups=%d two_sets=%d list_words=%zu rank_words=%zu traced=%zu traced_words=%zu\n", k.name, n_long, n_jobs,
           p.n_part, p.group, p.n_groups, p.two_sets ? 1 : 0, p.sec_list_words, p.sec_rank_words, p.sec_traced(), p.sec_traced_words());
    CHECK(p.sec_list_words == n_long * n_jobs * 15, "%s: a list of 15 words per (read, job) pair", k.name);
    CHECK(p.sec_rank_words == 25 * n_long, "%s: five arrays of five ranks per long read", k.name);
    if (n_long == 0) return;
    // every (array, rank, read) has a word of its own inside the buffer; reads of one rank are consecutive (a group's part of a
    // rank is a plain pointer offset), ranks of one array n_long apart (rank k of a kernel's arrays: + k * n_long)
    std::set<size_t> seen;
    const sfa::LongPlan::SecArray arrays[5] = {p.kSecJob, p.kSecCol, p.kSecScore, p.kSecStart, p.kSecEnd};
    for (int a = 0; a < 5; ++a)
        for (int r = 0; r < sfa::kSecRanks; ++r)
            for (size_t li = 0; li < n_long; ++li) {
                const size_t w = p.sec_rank(arrays[a], r, static_cast<int32_t>(li));
                CHECK(w < p.sec_rank_words, "%s: word %zu outside the buffer", k.name, w);
                CHECK(seen.insert(w).second, "%s: word %zu used twice", k.name, w);
                CHECK(w == p.sec_rank(arrays[a], 0) + r * n_long + li, "%s: rank stride", k.name);
            }
    CHECK(seen.size() == p.sec_rank_words, "%s: the arrays fill the buffer", k.name);
    // the traced columns (start, end) are the tail of the buffer: one fill sets all of them to -1
    CHECK(p.sec_traced() == p.sec_rank(p.kSecStart, 0) && p.sec_rank(p.kSecEnd, 0) == p.sec_traced() + 5 * n_long, "%s: traced columns", k.name);
    CHECK(p.sec_traced() + p.sec_traced_words() == p.sec_rank_words && p.sec_traced_words() == 10 * n_long, "%s: traced words", k.name);
    // the groups' parts: group gi owns reads begin(gi) .. begin(gi) + size(gi) - 1 of every rank and the lists of their pairs
    size_t covered = 0;
    for (int32_t gi = 0; gi < p.n_groups; ++gi) {
        CHECK(static_cast<size_t>(p.begin(gi)) == covered, "%s: group %d begins where the one before ends", k.name, gi);
        covered += p.size(gi);
        CHECK((static_cast<size_t>(p.begin(gi)) + p.size(gi)) * n_jobs * sfa::kSecListWords <= p.sec_list_words, "%s: lists of group %d", k.name, gi);
    }
    CHECK(covered == n_long, "%s: the groups cover the long reads", k.name);
}

int main() {
    const std::vector<int32_t> ncov = {29898, 29898}, four = {2600, 2600, 700, 700};
    const int64_t ample = 16ll << 30;
    // one read's scratch on `four` at 3 strips, T = 512: two boundary rows of all jobs' padded columns, 3 x ((len - 1) >> 9) records per job
    const int64_t per_read = 4 * 2 * 2 * (2856 + 956) + 4ll * sfa::kCkRec * 3 * 2 * (5 + 1);
    const std::vector<Case> cases = {
        {"none", ncov, {250, 2048, 0}, 0, ample},
        {"one", ncov, {2049}, 0, ample},
        {"mixed", ncov, {250, 2049, 6500, 2048, 4097}, 0, ample},
        {"three_groups", four, {2049, 3000, 250, 4097, 2500, 3585, 2100}, 512, 4 * per_read},
        {"one_per_group", four, {2049, 3000, 4097}, 512, 1},
    };
    for (const Case &k : cases) run(k);
    printf("done %d\n", failures);
    return failures ? 1 : 0;
}
