// The host rules of a session's group cap (sigfish_amd/csrc/group_cover_rules.hpp, the header sfa_session_targets.hip and the kernels of
// sdtw_session_groupcover.hpp share) as a stand-alone host program, built from that header alone; tests/test_session_group_cover_cpu.py
// runs it plain and under ASan + UBSan and compares its answers with the numpy model of tests/group_cover_model.py.
//   selftest      the rule at its edges: depth cap - 1 open and cap closed side by side, a background column at any depth, a column
//                 two groups cover whose coordinate is capped (background, not the higher group), the records over '+' only, an
//                 empty group, the firsts handed to open_first_cols.  Prints "selftest ok <cases>".
//   labels <strands> <num_ref> <len, offset per contig> <n_groups> <cap> <n> <contig begin end group per target> <m> <contig begin end per interval>
//                 "refused <text>" when either list is, else
//                 "live <columns of a group> <label per column ...>", "first <column per entry ...>", one line
//                 "rec <entry> <columns> <capped> <sum> <min> <max>" per entry, "base <label per column ...>" and
//                 "open <first on> <first off>" (open_first_cols under a bitmap with every EVEN group open)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "group_cover_rules.hpp"
#include "quota_rules.hpp"

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
    const std::vector<int32_t> lens = {7, 5}, offs = {10, 0};
    for (int strands = 1; strands <= 2; ++strands) {
        const Model md(lens, offs, strands);
        // groups 0 and 2 overlap on coordinates 12 .. 13 of contig 0; group 1 has no interval; group 3 is contig 1's
        const sfa_group_target_t t[] = {{0, 11, 14, 0}, {0, 12, 16, 2}, {1, 0, 6, 3}};
        const int32_t n_groups = 4;
        std::vector<uint16_t> base, live;
        std::vector<int32_t> first;
        sfa::group_labels(t, 3, n_groups, md.m, &base);
        std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off.back()), 0u);
        // depth 0: the live table is the base table
        int64_t in = sfa::group_cover_live_labels(base, depth.data(), md.cov_off.data(), 2, n_groups, md.m, &live, &first);
        CHECK(live == base && in == strands * (5 + 5));  // five labelled coordinates per contig, each on every strand
        CHECK(first[0] == 1 && first[2] == 4 && first[1] == sfa::kNoColumn && first[4] == 0 && first[3] == strands * 7);
        // coordinate 12 to depth 1 (cap - 1: open) and 13 to depth 2 (cap: closed), side by side
        const sfa_target_t iv[] = {{0, 12, 14}, {0, 13, 14}};
        sfa::coverage_add(iv, 2, md.m, md.cov_off.data(), depth.data());
        in = sfa::group_cover_live_labels(base, depth.data(), md.cov_off.data(), 2, n_groups, md.m, &live, &first);
        CHECK(live[2] == 0 && live[3] == 4);  // '+' columns 2, 3: group 0 stays at depth 1; at depth 2 the column goes to the background, NOT to group 2
        CHECK(base[3] == 0 && live[4] == 2 && live[5] == 2);
        if (strands == 2) CHECK(live[7 + 7 - 3] == 4 && live[7 + 7 - 2] == 0);  // '-' column 4 is coordinate 13, column 5 coordinate 12
        CHECK(in == strands * 10 - strands);
        // a background column stays background at any depth, and at depth 0
        CHECK(sfa::group_live_label(4, depth.data(), '+', 0, 7, 10, 1u, 4) == 4 && sfa::group_live_label(4, depth.data(), '+', 3, 7, 10, 1000u, 4) == 4);
        CHECK(sfa::group_live_label(0, depth.data(), '+', 3, 7, 10, 3u, 4) == 0 && sfa::group_live_label(0, depth.data(), '+', 3, 7, 10, 2u, 4) == 4);
        // the records: '+' columns only, by BASE label -- coordinate 13 still counts for group 0
        std::vector<sfa_group_cover_t> rec;
        sfa::group_cover_records(base, depth.data(), md.cov_off.data(), 2, n_groups, md.m, &rec);
        CHECK(rec.size() == 5 && rec[0].columns == 3 && rec[0].capped == 1 && rec[0].depth_sum == 3 && rec[0].depth_min == 0 && rec[0].depth_max == 2);
        CHECK(rec[2].columns == 2 && rec[2].capped == 0 && rec[2].depth_sum == 0 && rec[2].depth_min == 0 && rec[2].depth_max == 0);
        CHECK(rec[1].columns == 0 && rec[1].capped == 0 && rec[1].depth_sum == 0 && rec[1].depth_min == UINT32_MAX && rec[1].depth_max == 0);  // the empty group
        CHECK(rec[3].columns == 5 && rec[4].columns == 2);  // (coordinate 5 of contig 1, which only '-' reports, is nobody's)
        // every column of group 3 capped: its first goes, and open_first_cols sees a label without columns
        const sfa_target_t all1[] = {{1, 0, 6}, {1, 0, 6}};
        sfa::coverage_add(all1, 2, md.m, md.cov_off.data(), depth.data());
        sfa::group_cover_live_labels(base, depth.data(), md.cov_off.data(), 2, n_groups, md.m, &live, &first);
        CHECK(first[3] == sfa::kNoColumn);
        std::vector<int32_t> for_open;
        sfa::group_cover_firsts_for_open(first.data(), n_groups, &for_open);
        CHECK(for_open[3] == -1 && for_open[1] == -1 && for_open[0] == 1);
        uint32_t norm[sfa::kOpenWords];
        const uint32_t only3 = 1u << 3;
        sfa::open_normalise(&only3, n_groups, norm);
        int32_t on, off;
        sfa::open_first_cols(for_open, n_groups, norm, &on, &off);
        CHECK(on == -1 && off == 0);  // the ON class is empty: the class falls back as the open call documents
        sfa::group_cover_records(base, depth.data(), md.cov_off.data(), 2, n_groups, md.m, &rec);
        CHECK(rec[3].columns == 5 && rec[3].capped == 5 && rec[3].depth_min == 2 && rec[3].depth_sum == 10);
        CHECK(sfa::group_cover_bytes(md.m.total_cols, n_groups) == 8 * sfa::group_label_words(md.m.total_cols) + 36 * 5);
    }
    printf("selftest ok %d\n", n_cases);
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest")) {
            selftest();
        } else if (!strcmp(word, "labels")) {
            int strands, num_ref, n_groups, cap, n, k;
            if (scanf("%d %d", &strands, &num_ref) != 2 || num_ref < 1) return 2;
            std::vector<int32_t> lens(num_ref), offs(num_ref);
            for (int r = 0; r < num_ref; ++r)
                if (scanf("%d %d", &lens[r], &offs[r]) != 2) return 2;
            if (scanf("%d %d %d", &n_groups, &cap, &n) != 3 || n < 0) return 2;
            std::vector<sfa_group_target_t> t(static_cast<size_t>(n));
            for (sfa_group_target_t &x : t)
                if (scanf("%d %d %d %d", &x.contig, &x.begin, &x.end, &x.group) != 4) return 2;
            if (scanf("%d", &k) != 1 || k < 0) return 2;
            std::vector<sfa_target_t> iv(static_cast<size_t>(k));
            for (sfa_target_t &x : iv)
                if (scanf("%d %d %d", &x.contig, &x.begin, &x.end) != 3) return 2;
            const Model md(lens, offs, strands);
            char msg[256];
            if (const char *why = sfa::group_list_error(t.data(), n, n_groups, md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            if (const char *why = sfa::coverage_list_error(iv.data(), k, md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            std::vector<uint16_t> base, live;
            std::vector<int32_t> first, for_open;
            std::vector<sfa_group_cover_t> rec;
            std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off.back()), 0u);
            sfa::group_labels(t.data(), n, n_groups, md.m, &base);
            sfa::coverage_add(iv.data(), k, md.m, md.cov_off.data(), depth.data());
            const int64_t in = sfa::group_cover_live_labels(base, depth.data(), md.cov_off.data(), static_cast<uint32_t>(cap), n_groups, md.m, &live, &first);
            sfa::group_cover_records(base, depth.data(), md.cov_off.data(), static_cast<uint32_t>(cap), n_groups, md.m, &rec);
            printf("live %lld", static_cast<long long>(in));
            for (int64_t c = 0; c < md.m.total_cols; ++c) printf(" %u", live[static_cast<size_t>(c)]);
            printf("\nfirst");
            for (const int32_t f : first) printf(" %d", f);
            printf("\n");
            for (size_t e = 0; e < rec.size(); ++e)
                printf("rec %zu %lld %lld %llu %u %u\n", e, static_cast<long long>(rec[e].columns), static_cast<long long>(rec[e].capped),
                       static_cast<unsigned long long>(rec[e].depth_sum), rec[e].depth_min, rec[e].depth_max);
            printf("base");
            for (int64_t c = 0; c < md.m.total_cols; ++c) printf(" %u", base[static_cast<size_t>(c)]);
            printf("\n");
            for (size_t c = static_cast<size_t>(md.m.total_cols); c < live.size(); ++c)
                if (live[c] != n_groups) return 3;  // the padding holds the background
            std::vector<uint32_t> even(static_cast<size_t>(sfa::open_words(n_groups)), 0x55555555u);
            uint32_t norm[sfa::kOpenWords];
            sfa::open_normalise(even.data(), n_groups, norm);
            sfa::group_cover_firsts_for_open(first.data(), n_groups, &for_open);
            int32_t on, off;
            sfa::open_first_cols(for_open, n_groups, norm, &on, &off);
            printf("open %d %d\n", on, off);
        } else {
            return 2;
        }
    }
    return 0;
}
