// The host rules of a session's target classes (sigfish_amd/csrc/target_rules.hpp, the header sfa_session_targets.hip builds its mask and
// decides with) as a stand-alone host program, built from that header alone; tests/test_session_targets_cpu.py runs it plain and
// under ASan + UBSan.
//   selftest                      the mask of every case against a loop that calls place_col (row_rules.hpp) for every column and
//                                 every interval; every refusal; the decision table.  Prints "selftest ok <cases>".
//   mask <strands> <num_ref> <len, offset per contig> <n> <contig begin end per target>
//                                 "refused <text>", or "mask <on columns> <first on> <first off> <words in hex ...>"
//   decide <on_score> <off_score> <on_rid> <off_rid> <n_events> <valid> <mode> <min_events> <margin>
//                                 "decide A" / "decide U" / "decide -"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "target_rules.hpp"

namespace {

struct Model {
    std::vector<int32_t> job_contig, job_len, ref_len, ref_off;
    std::vector<int8_t> job_strand;
    std::vector<int64_t> col_off;
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
    }
};

// every column against every interval, through place_col
std::vector<uint32_t> brute(const Model &md, const std::vector<sfa_target_t> &t, int64_t *on) {
    std::vector<uint32_t> mask(sfa::target_mask_words(md.m.total_cols), 0u);
    *on = 0;
    for (int32_t j = 0; j < md.m.n_jobs; ++j)
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const int32_t r = md.job_contig[j];
            const int x = sfa::place_col(md.job_strand[j], col, md.ref_len[r], md.ref_off[r]);
            bool hit = false;
            for (const sfa_target_t &k : t) hit = hit || (k.contig == r && k.begin <= x && x < k.end);
            if (hit) {
                const int64_t g = md.col_off[j] + col;
                mask[static_cast<size_t>(g >> 5)] |= 1u << (g & 31);
                ++*on;
            }
        }
    return mask;
}

int n_cases = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

void check_mask(const Model &md, const std::vector<sfa_target_t> &t) {
    char msg[192];
    CHECK(sfa::target_list_error(t.data(), static_cast<int32_t>(t.size()), md.m, msg, sizeof msg) == nullptr);
    std::vector<uint32_t> got;
    int64_t want_on = 0;
    const int64_t on = sfa::target_mask(t.data(), static_cast<int32_t>(t.size()), md.m, &got);
    const std::vector<uint32_t> want = brute(md, t, &want_on);
    CHECK(got == want && on == want_on);
    int32_t first_on = -1, first_off = -1;
    for (int64_t g = md.m.total_cols - 1; g >= 0; --g) ((want[static_cast<size_t>(g >> 5)] >> (g & 31)) & 1 ? first_on : first_off) = static_cast<int32_t>(g);
    CHECK(sfa::target_first_of_class(got, md.m.total_cols, true) == first_on && sfa::target_first_of_class(got, md.m.total_cols, false) == first_off);
    ++n_cases;
}

void refused(const Model &md, sfa_target_t t, const char *word) {
    char msg[192];
    const char *why = sfa::target_list_error(&t, 1, md.m, msg, sizeof msg);
    CHECK(why != nullptr && strstr(why, word) != nullptr);
    ++n_cases;
}

sfa_class_t cls(float on, float off, int32_t on_rid, int32_t off_rid, int32_t n, int32_t valid = 1) {
    sfa_class_t c;
    memset(&c, 0, sizeof c);
    c.on_score = on, c.off_score = off, c.on_rid = on_rid, c.off_rid = off_rid, c.n_events = n, c.valid = valid;
    c.on_pos_end = on_rid < 0 ? -1 : 5, c.off_pos_end = off_rid < 0 ? -1 : 7;
    return c;
}

void selftest() {
    const std::vector<int32_t> lens = {1, 31, 32, 33, 64, 65, 300};
    for (int strands = 1; strands <= 2; ++strands)  // 1: RNA, the forward arrays only
        for (int shift = 0; shift < 2; ++shift) {
            std::vector<int32_t> offs(lens.size(), 0);
            if (shift) offs = {0, 7, 0, 100, 3, 0, 1000};
            const Model md(lens, offs, strands);
            check_mask(md, {});  // the empty list: nothing on target
            for (int32_t r = 0; r < md.m.num_ref; ++r) {
                const int32_t off = offs[r], rl = lens[r];
                check_mask(md, {{r, off, off + rl + 1}});  // the whole contig, both ends of both strands
                check_mask(md, {{r, off, off + 1}});
                check_mask(md, {{r, off + rl, off + rl + 1}});
                check_mask(md, {{r, off + rl - 1, off + rl}});
                // intervals that begin or end where a word of the mask does: in every job of the contig, for either direction
                for (int32_t j = 0; j < md.m.n_jobs; ++j) {
                    if (md.job_contig[j] != r) continue;
                    for (int64_t edge = (md.col_off[j] + 31) / 32 * 32; edge <= md.col_off[j] + rl; edge += 32) {
                        const int32_t col = static_cast<int32_t>(edge - md.col_off[j]);
                        for (int32_t c2 : {col - 1, col, col + 1}) {
                            if (c2 < 0 || c2 >= rl) continue;
                            const int x = sfa::place_col(md.job_strand[j], c2, rl, off);
                            if (x >= 1) check_mask(md, {{r, x > 3 ? x - 3 : 0, x}});       // ends at it
                            check_mask(md, {{r, x, x + 3 < off + rl + 1 ? x + 3 : off + rl + 1}});  // begins at it
                            check_mask(md, {{r, x, x + 1}});
                        }
                    }
                }
            }
            // overlapping, touching, unsorted, on several contigs
            check_mask(md, {{6, offs[6] + 200, offs[6] + 260}, {6, offs[6] + 10, offs[6] + 40}, {6, offs[6] + 30, offs[6] + 64}, {6, offs[6] + 64, offs[6] + 65},
                            {3, offs[3] + 5, offs[3] + 20}, {1, offs[1], offs[1] + 32}, {6, offs[6] + 10, offs[6] + 40}, {4, offs[4] + 63, offs[4] + 65}});
            // every refusal
            refused(md, {-1, 0, 1}, "contig");
            refused(md, {7, 0, 1}, "contig");
            refused(md, {2, -1, 4}, "negative");
            refused(md, {2, 4, 4}, "empty");
            refused(md, {2, 5, 4}, "empty");
            refused(md, {2, 0, offs[2] + 32 + 2}, "beyond");
            refused(md, {0, 0, offs[0] + 3}, "beyond");
        }
    // the decision table
    const float inf = INFINITY;
    struct Row {
        sfa_class_t c;
        int mode, min_events;
        float margin;
        char want;
    };
    const Row table[] = {
        {cls(10.f, 60.f, 0, 1, 100), 0, 100, 0.5f, 'A'},   // margin exactly met (50 = 0.5 * 100), n at min_events: on target, enrich
        {cls(10.f, 60.f, 0, 1, 100), 1, 100, 0.5f, 'U'},   // ... deplete
        {cls(10.f, 60.f, 0, 1, 99), 0, 100, 0.5f, 0},      // n just below min_events
        {cls(10.f, 59.5f, 0, 1, 100), 0, 100, 0.5f, 0},    // margin just missed
        {cls(60.f, 10.f, 0, 1, 100), 0, 100, 0.5f, 'U'},   // off target exactly met
        {cls(60.f, 10.f, 0, 1, 100), 1, 100, 0.5f, 'A'},
        {cls(59.5f, 10.f, 0, 1, 100), 1, 100, 0.5f, 0},
        {cls(inf, 10.f, -1, 1, 100), 0, 100, 0.5f, 'U'},   // no column on target
        {cls(inf, 10.f, -1, 1, 100), 1, 100, 0.5f, 'A'},
        {cls(10.f, inf, 0, -1, 100), 0, 100, 0.5f, 'A'},   // no column off target
        {cls(10.f, inf, 0, -1, 100), 1, 100, 0.5f, 'U'},
        {cls(inf, inf, -1, -1, 100), 0, 100, 0.5f, 0},     // both empty
        {cls(inf, inf, -1, -1, 100), 1, 100, 0.5f, 0},
        {cls(3.f, 10.f, -1, 1, 100), 0, 100, 0.5f, 'U'},   // an empty class counts as +inf whatever its score field holds
        {cls(10.f, 60.f, 0, 1, 100, 0), 0, 100, 0.5f, 0},  // valid = 0
        {cls(10.f, 60.f, 0, 1, 100), 2, 100, 0.5f, 0},     // an unknown mode
        {cls(10.f, 60.f, 0, 1, 100), 0, 100, -1.f, 0},     // a negative margin
        {cls(10.f, 10.f, 0, 1, 100), 0, 100, 0.f, 'A'},    // margin 0 and equal scores: on target is asked first
    };
    for (const Row &r : table) {
        CHECK(sfa::target_decide(r.c, r.mode, r.min_events, r.margin) == r.want);
        ++n_cases;
    }
    // the order of partial minima and the placing of a column
    CHECK(sfa::class_before(1.f, 9, 2.f, 3) && !sfa::class_before(2.f, 3, 1.f, 9) && sfa::class_before(1.f, 3, 1.f, 9) && !sfa::class_before(1.f, 9, 1.f, 9));
    CHECK(sfa::class_before(inf, 3, inf, sfa::kNoColumn) && !sfa::class_before(inf, sfa::kNoColumn, inf, sfa::kNoColumn));
    {
        const Model md(lens, {0, 7, 0, 100, 3, 0, 1000}, 2);
        const sfa::RefTables t{md.job_contig.data(), md.job_strand.data(), md.ref_len.data(), md.ref_off.data()};
        for (int32_t j = 0; j < md.m.n_jobs; ++j)
            for (int32_t col : {0, md.job_len[j] - 1}) {
                const sfa::ClassPlace p = sfa::class_place(static_cast<int32_t>(md.col_off[j] + col), md.m.n_jobs, md.col_off.data(), t);
                const int32_t r = md.job_contig[j];
                CHECK(p.rid == r && p.strand == md.job_strand[j] && p.pos_end == sfa::place_col(md.job_strand[j], col, md.ref_len[r], md.ref_off[r]));
                ++n_cases;
            }
        const sfa::ClassPlace none = sfa::class_place(sfa::kNoColumn, md.m.n_jobs, md.col_off.data(), t);
        CHECK(none.rid == -1 && none.pos_end == -1 && none.strand == 0);
    }
    printf("selftest ok %d\n", n_cases);
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest")) {
            selftest();
        } else if (!strcmp(word, "mask")) {
            int strands, num_ref, n;
            if (scanf("%d %d", &strands, &num_ref) != 2) return 2;
            std::vector<int32_t> lens(num_ref), offs(num_ref);
            for (int r = 0; r < num_ref; ++r)
                if (scanf("%d %d", &lens[r], &offs[r]) != 2) return 2;
            if (scanf("%d", &n) != 1) return 2;
            std::vector<sfa_target_t> t(n);
            for (int k = 0; k < n; ++k)
                if (scanf("%d %d %d", &t[k].contig, &t[k].begin, &t[k].end) != 3) return 2;
            const Model md(lens, offs, strands);
            char msg[192];
            if (const char *why = sfa::target_list_error(t.data(), n, md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            std::vector<uint32_t> mask;
            const int64_t on = sfa::target_mask(t.data(), n, md.m, &mask);
            printf("mask %lld %d %d", static_cast<long long>(on), sfa::target_first_of_class(mask, md.m.total_cols, true), sfa::target_first_of_class(mask, md.m.total_cols, false));
            for (size_t w = 0; w + 1 < mask.size(); ++w) printf(" %08x", mask[w]);
            printf("\n");
        } else if (!strcmp(word, "decide")) {
            float on, off, margin;
            int on_rid, off_rid, n, valid, mode, min_events;
            if (scanf("%f %f %d %d %d %d %d %d %f", &on, &off, &on_rid, &off_rid, &n, &valid, &mode, &min_events, &margin) != 9) return 2;
            const char d = sfa::target_decide(cls(on, off, on_rid, off_rid, n, valid), mode, min_events, margin);
            printf("decide %c\n", d ? d : '-');
        } else {
            return 2;
        }
    }
    return 0;
}
