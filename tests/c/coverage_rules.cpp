// The host rules of a session's coverage cap (sigfish_amd/csrc/coverage_rules.hpp, the header sfa_session_targets.hip and the kernels of
// sdtw_session_cover.hpp share) as a stand-alone host program, built from that header alone; tests/test_session_coverage_cpu.py
// runs it plain and under ASan + UBSan and compares its answers with the numpy model of tests/coverage_model.py.
//   selftest      the layout (coverage_offsets, coverage_span's clipping, coverage_entry at both ends of both strands), depth cap - 1
//                 open and cap closed on one coordinate, 300 copies of an interval.  Prints "selftest ok <cases>".
//   live <strands> <num_ref> <len, offset per contig> <cap> <n> <contig begin end per target> <m> <contig begin end per interval>
//                 "refused <text>" when either list is (the intervals through coverage_list_error), else
//                 "live <live columns> <first on> <first off> <words in hex ...>", then one line "depth <contig> <entries ...>" per
//                 contig and "base <words in hex ...>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "coverage_rules.hpp"

namespace {

struct Model {
    std::vector<int32_t> job_contig, job_len, ref_len, ref_off;
    std::vector<int8_t> job_strand;
    std::vector<int64_t> col_off, cov_off;
    sfa::TargetModel m;
    Model(const std::vector<int32_t> &lens, const std::vector<int32_t> &offs, int strands) : ref_len(lens), ref_off(offs) {
        int64_t total = 0;
        for (size_t r = 0; r < lens.size(); ++r)
            for (int s = 0; s < strands; ++s) {
                job_contig.push_back(static_cast<int32_t>(r));
                job_strand.push_back(s ? '-' : '+');
                job_len.push_back(lens[r]);
                col_off.push_back(total);
                total += lens[r];
            }
        m = sfa::TargetModel{static_cast<int32_t>(lens.size()), static_cast<int32_t>(job_len.size()), job_contig.data(), job_strand.data(), job_len.data(),
                             col_off.data(),                    ref_len.data(),                       ref_off.data(),    total};
        sfa::coverage_offsets(ref_len.data(), m.num_ref, &cov_off);
    }
};

int n_cases = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                 \
        }                                                            \
        ++n_cases;                                                   \
    } while (0)

void selftest() {
    const std::vector<int32_t> lens = {1, 31, 33, 70}, offs = {0, 7, 100, 3};
    for (int strands = 1; strands <= 2; ++strands) {
        const Model md(lens, offs, strands);
        // the layout: ref_len + 1 entries per contig, back to back
        CHECK(md.cov_off.size() == 5 && md.cov_off[0] == 0 && md.cov_off[1] == 2 && md.cov_off[2] == 34 && md.cov_off[3] == 68 && md.cov_off[4] == 139);
        CHECK(sfa::coverage_bytes(md.cov_off[4], md.m.total_cols) == 4 * 139 + 4 * sfa::target_mask_words(md.m.total_cols));
        for (int32_t r = 0; r < md.m.num_ref; ++r) {
            const int32_t rl = lens[r], off = offs[r];
            // a column's entry: 0 .. rl - 1 along '+', rl .. 1 along '-'
            CHECK(sfa::coverage_entry('+', 0, rl, off) == 0 && sfa::coverage_entry('+', rl - 1, rl, off) == rl - 1);
            CHECK(sfa::coverage_entry('-', 0, rl, off) == rl && sfa::coverage_entry('-', rl - 1, rl, off) == 1);
            // an interval's entries, clipped to the track
            sfa::CoverSpan s = sfa::coverage_span(off, off + rl + 1, rl, off);
            CHECK(s.lo == 0 && s.hi == rl + 1);
            s = sfa::coverage_span(0, off + 1, rl, off);  // begins below the offset: only coordinate off counts
            CHECK(s.lo == 0 && s.hi == 1);
            s = sfa::coverage_span(0, off, rl, off);  // wholly below it: nothing
            CHECK(s.lo >= s.hi);
            s = sfa::coverage_span(off + rl, INT32_MAX, rl, off);  // (a list that passed coverage_list_error never ends beyond; clipped all the same)
            CHECK(s.lo == rl && s.hi == rl + 1);
            s = sfa::coverage_span(INT32_MAX - 1, INT32_MAX, rl, off);
            CHECK(s.lo >= s.hi);
        }
        // cap - 1 is open, cap is closed, on the same coordinate; 300 copies of an interval leave + 300
        std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off[4]), 0u), base, live;
        const sfa_target_t whole = {3, offs[3], offs[3] + lens[3] + 1};
        const int64_t on = sfa::target_mask(&whole, 1, md.m, &base);
        CHECK(on == strands * lens[3]);
        CHECK(sfa::coverage_live_mask(base, depth.data(), md.cov_off.data(), 300, md.m, &live) == on && live == base);
        const std::vector<sfa_target_t> copies(299, sfa_target_t{3, offs[3] + 10, offs[3] + 11});
        sfa::coverage_add(copies.data(), 299, md.m, md.cov_off.data(), depth.data());
        CHECK(depth[static_cast<size_t>(md.cov_off[3]) + 10] == 299 && depth[static_cast<size_t>(md.cov_off[3]) + 9] == 0 && depth[static_cast<size_t>(md.cov_off[3]) + 11] == 0);
        CHECK(sfa::coverage_live_mask(base, depth.data(), md.cov_off.data(), 300, md.m, &live) == on);
        sfa::coverage_add(copies.data(), 1, md.m, md.cov_off.data(), depth.data());
        CHECK(sfa::coverage_live_mask(base, depth.data(), md.cov_off.data(), 300, md.m, &live) == on - strands);  // the coordinate closes on both strands
        CHECK(live.back() == 0u);                                                                                  // the spare word
        CHECK(sfa::coverage_live_mask(base, depth.data(), md.cov_off.data(), 301, md.m, &live) == on);
        // the rule itself: an off-target column is never live, whatever its depth
        CHECK(!sfa::coverage_live(false, depth.data(), '+', 0, lens[0], offs[0], 1u) && sfa::coverage_live(true, depth.data(), '+', 0, lens[0], offs[0], 1u));
        // the refusals are a target list's
        char msg[192];
        const sfa_target_t bad[] = {{-1, 0, 1}, {4, 0, 1}, {2, -1, 4}, {2, 4, 4}, {2, 0, offs[2] + lens[2] + 2}};
        const char *word[] = {"contig", "contig", "negative", "empty", "beyond"};
        for (int k = 0; k < 5; ++k) {
            const char *why = sfa::coverage_list_error(&bad[k], 1, md.m, msg, sizeof msg);
            CHECK(why != nullptr && strstr(why, word[k]) != nullptr && strstr(why, "target 0:") != nullptr);
        }
    }
    printf("selftest ok %d\n", n_cases);
}

bool read_list(std::vector<sfa_target_t> *t) {
    int n;
    if (scanf("%d", &n) != 1 || n < 0) return false;
    t->resize(static_cast<size_t>(n));
    for (sfa_target_t &x : *t)
        if (scanf("%d %d %d", &x.contig, &x.begin, &x.end) != 3) return false;
    return true;
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest")) {
            selftest();
        } else if (!strcmp(word, "live")) {
            int strands, num_ref, cap;
            if (scanf("%d %d", &strands, &num_ref) != 2) return 2;
            std::vector<int32_t> lens(num_ref), offs(num_ref);
            for (int r = 0; r < num_ref; ++r)
                if (scanf("%d %d", &lens[r], &offs[r]) != 2) return 2;
            std::vector<sfa_target_t> t, iv;
            if (scanf("%d", &cap) != 1 || !read_list(&t) || !read_list(&iv)) return 2;
            const Model md(lens, offs, strands);
            char msg[192];
            if (const char *why = sfa::target_list_error(t.data(), static_cast<int32_t>(t.size()), md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            if (const char *why = sfa::coverage_list_error(iv.data(), static_cast<int32_t>(iv.size()), md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            std::vector<uint32_t> base, live, depth(static_cast<size_t>(md.cov_off.back()), 0u);
            sfa::target_mask(t.data(), static_cast<int32_t>(t.size()), md.m, &base);
            sfa::coverage_add(iv.data(), static_cast<int32_t>(iv.size()), md.m, md.cov_off.data(), depth.data());
            const int64_t n_live = sfa::coverage_live_mask(base, depth.data(), md.cov_off.data(), static_cast<uint32_t>(cap), md.m, &live);
            printf("live %lld %d %d", static_cast<long long>(n_live), sfa::target_first_of_class(live, md.m.total_cols, true), sfa::target_first_of_class(live, md.m.total_cols, false));
            for (size_t w = 0; w + 1 < live.size(); ++w) printf(" %08x", live[w]);
            printf("\n");
            for (int r = 0; r < num_ref; ++r) {
                printf("depth %d", r);
                for (int64_t e = md.cov_off[r]; e < md.cov_off[r + 1]; ++e) printf(" %u", depth[static_cast<size_t>(e)]);
                printf("\n");
            }
            printf("base");
            for (size_t w = 0; w + 1 < base.size(); ++w) printf(" %08x", base[w]);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
