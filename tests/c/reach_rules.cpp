// The host rules of a session's reach targets (sigfish_amd/csrc/reach_rules.hpp, the header sfa_session_targets.hip and the kernels of
// sdtw_session_reach.hpp share) as a stand-alone host program, built from that header alone; tests/test_reach_model_cpu.py runs
// it plain and under ASan + UBSan and compares its answers with the numpy model of tests/reach_model.py.
//   selftest      the list refusals; reach_tables against a second, brute-force statement (per column over every target, the
//                 admitting set spelled out); lead 0 / strand 0 equal to target_mask with anchor x; the prepared runs bisected on
//                 the host equal to the tables, on crafted and on random lists.  Prints "selftest ok <cases>".
//   reach <strands> <num_ref> <len, offset per contig> <cap> <n> <contig begin end lead strand per target (strand . + -)>
//         <m> <contig begin end per coverage interval>
//                 "refused <text>" when either list is, else
//                 "mask <on columns> <words in hex ...>", "anchor <coordinate per column ...>" (reach_tables),
//                 "entry <entry per column ...>" (the prepared runs, bisected), "live <live columns> <words in hex ...>"
//                 (reach_live_mask under the depth the intervals leave and the cap)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "reach_rules.hpp"

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

sfa_reach_target_t rt(int32_t contig, int32_t begin, int32_t end, int32_t lead, int strand) {
    sfa_reach_target_t t{};
    t.contig = contig, t.begin = begin, t.end = end, t.lead = lead, t.strand = static_cast<int8_t>(strand);
    return t;
}

// the second statement: the admitting set of a column spelled out from the issue's two inequalities, in 64 bits
void brute(const std::vector<sfa_reach_target_t> &t, const Model &md, std::vector<uint32_t> *mask, std::vector<int32_t> *anchor) {
    mask->assign(sfa::target_mask_words(md.m.total_cols), 0u);
    anchor->assign(static_cast<size_t>(md.m.total_cols), -1);
    for (int32_t j = 0; j < md.m.n_jobs; ++j) {
        const int32_t c = md.job_contig[j], rl = md.ref_len[c], off = md.ref_off[c];
        const bool plus = md.job_strand[j] == '+';
        for (int32_t col = 0; col < rl; ++col) {
            const long long x = plus ? static_cast<long long>(col) + off : static_cast<long long>(rl) - col + off;
            std::vector<long long> cand;
            for (const sfa_reach_target_t &q : t) {
                if (q.contig != c) continue;
                if (q.strand == '+' && !plus) continue;
                if (q.strand == '-' && plus) continue;
                const long long b = q.begin, e = q.end, l = q.lead;
                if (plus && b - l <= x && x < e) cand.push_back(x > b ? x : b);
                if (!plus && b <= x && x < e + l) cand.push_back(x < e - 1 ? x : e - 1);
            }
            if (cand.empty()) continue;
            long long best = cand[0];
            for (const long long v : cand) best = plus ? (v < best ? v : best) : (v > best ? v : best);
            const int64_t g = md.col_off[j] + col;
            (*mask)[static_cast<size_t>(g >> 5)] |= 1u << (g & 31);
            (*anchor)[static_cast<size_t>(g)] = static_cast<int32_t>(best);
        }
    }
}

// reach_tables == brute, and the prepared runs, bisected, give the same mask and the anchors as entries
void check_list(const std::vector<sfa_reach_target_t> &t, const Model &md) {
    char msg[224];
    CHECK(sfa::reach_list_error(t.data(), static_cast<int32_t>(t.size()), md.m, msg, sizeof msg) == nullptr);
    std::vector<uint32_t> mask, mask2, mask3;
    std::vector<int32_t> anchor, anchor2, entry;
    const int64_t on = sfa::reach_tables(t.data(), static_cast<int32_t>(t.size()), md.m, &mask, &anchor);
    brute(t, md, &mask2, &anchor2);
    CHECK(mask == mask2);
    CHECK(anchor == anchor2);
    sfa::ReachPrepared p;
    sfa::reach_prepare(t.data(), static_cast<int32_t>(t.size()), md.m, &p);
    CHECK(sfa::reach_tables_from_runs(p, md.m, &mask3, &entry) == on);
    CHECK(mask3 == mask);
    CHECK(mask.back() == 0u);  // the spare word
    for (int32_t j = 0; j < md.m.n_jobs; ++j) {
        const int32_t c = md.job_contig[j];
        for (int32_t r = p.run_off[j]; r < p.run_off[j + 1]; ++r) {  // rising, disjoint, inside the job
            CHECK(p.runs[r].lo < p.runs[r].hi && p.runs[r].lo >= 0 && p.runs[r].hi <= md.job_len[j]);
            if (r > p.run_off[j]) CHECK(p.runs[r - 1].hi <= p.runs[r].lo);
        }
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const size_t g = static_cast<size_t>(md.col_off[j] + col);
            if (entry[g] != sfa::reach_entry_of(anchor[g], md.ref_off[c])) CHECK(false);
            if (entry[g] >= 0 && entry[g] > md.ref_len[c]) CHECK(false);  // inside the contig's track
        }
    }
    ++n_cases;
}

void selftest() {
    const std::vector<int32_t> lens = {1, 31, 33, 70}, offs = {0, 7, 100, 3};
    for (int strands = 1; strands <= 2; ++strands) {
        const Model md(lens, offs, strands);
        char msg[224];
        // ---- the refusals: a target list's, with its words and the target's number, then the fields of a reach target ----
        {
            const sfa_target_t bad[] = {{-1, 0, 1}, {4, 0, 1}, {2, -1, 4}, {2, 4, 4}, {2, 0, offs[2] + lens[2] + 2}};
            for (int k = 0; k < 5; ++k) {
                const sfa_target_t two[] = {{2, 100, 110}, bad[k]};
                char want[224];
                CHECK(sfa::target_list_error(two, 2, md.m, want, sizeof want) != nullptr);
                const sfa_reach_target_t list[] = {rt(2, 100, 110, 5, '+'), rt(bad[k].contig, bad[k].begin, bad[k].end, 0, 0)};
                const char *why = sfa::reach_list_error(list, 2, md.m, msg, sizeof msg);
                CHECK(why != nullptr && !strcmp(why, want));
            }
            sfa_reach_target_t x = rt(2, 100, 110, -1, 0);
            CHECK(strstr(sfa::reach_list_error(&x, 1, md.m, msg, sizeof msg), "lead") != nullptr);
            x = rt(2, 100, 110, sfa::kReachLeadMax + 1, 0);
            CHECK(strstr(sfa::reach_list_error(&x, 1, md.m, msg, sizeof msg), "lead") != nullptr);
            x = rt(2, 100, 110, sfa::kReachLeadMax, 0);
            CHECK(sfa::reach_list_error(&x, 1, md.m, msg, sizeof msg) == nullptr);
            x = rt(2, 100, 110, 0, 'x');
            CHECK(strstr(sfa::reach_list_error(&x, 1, md.m, msg, sizeof msg), "strand") != nullptr);
            x = rt(2, 100, 110, 0, 1);
            CHECK(strstr(sfa::reach_list_error(&x, 1, md.m, msg, sizeof msg), "strand") != nullptr);
            for (int b = 0; b < 3; ++b) {
                x = rt(2, 100, 110, 0, '-');
                x.pad[b] = 1;
                CHECK(strstr(sfa::reach_list_error(&x, 1, md.m, msg, sizeof msg), "padding") != nullptr);
            }
            // the count comes first: the list itself is not read
            CHECK(strstr(sfa::reach_list_error(nullptr, sfa::kReachTargetsMax + 1, md.m, msg, sizeof msg), "at most") != nullptr);
            const std::vector<sfa_reach_target_t> many(static_cast<size_t>(sfa::kReachTargetsMax), rt(3, 10, 11, 0, 0));
            CHECK(sfa::reach_list_error(many.data(), sfa::kReachTargetsMax, md.m, msg, sizeof msg) == nullptr);
        }
        // ---- lead 0, strand 0: target_mask word for word, anchor x ----
        {
            const std::vector<sfa_target_t> plain = {{1, 7, 12}, {1, 30, 39}, {2, 0, 101}, {2, 133, 134}, {3, 20, 30}, {3, 25, 40}, {3, 40, 41}, {0, 0, 2}};
            std::vector<sfa_reach_target_t> list;
            for (const sfa_target_t &q : plain) list.push_back(rt(q.contig, q.begin, q.end, 0, 0));
            std::vector<uint32_t> want, mask;
            std::vector<int32_t> anchor;
            const int64_t on = sfa::target_mask(plain.data(), static_cast<int32_t>(plain.size()), md.m, &want);
            CHECK(sfa::reach_tables(list.data(), static_cast<int32_t>(list.size()), md.m, &mask, &anchor) == on && mask == want);
            for (int32_t j = 0; j < md.m.n_jobs; ++j)
                for (int32_t col = 0; col < md.job_len[j]; ++col) {
                    const size_t g = static_cast<size_t>(md.col_off[j] + col);
                    const bool bit = (mask[g >> 5] >> (g & 31)) & 1u;
                    if (anchor[g] != (bit ? sfa::place_col(md.job_strand[j], col, md.ref_len[md.job_contig[j]], md.ref_off[md.job_contig[j]]) : -1)) CHECK(false);
                }
            check_list(list, md);
        }
        // ---- crafted lists ----
        check_list({}, md);
        check_list({rt(3, 40, 50, 10, '+')}, md);
        check_list({rt(3, 40, 50, 10, '-')}, md);
        check_list({rt(3, 40, 50, 10, 0)}, md);
        check_list({rt(3, 3, 4, 1 << 30, 0), rt(3, 73, 74, 1 << 30, 0)}, md);                    // first and last coordinate, the longest lead
        check_list({rt(2, 120, 125, 500, 0)}, md);                                               // a lead longer than the contig, below the offset
        check_list({rt(2, 0, 50, 30, 0), rt(2, 0, 100, 3, '-'), rt(2, 0, 101, 0, '-')}, md);     // bodies at and below the offset: kReachBelowTrack
        check_list({rt(3, 30, 35, 20, '+'), rt(3, 40, 45, 25, '+')}, md);                        // overlapping lead-ins: the nearer body
        check_list({rt(3, 30, 35, 5, '+'), rt(3, 40, 45, 40, '+')}, md);                         // a short lead nearer, a long one behind it
        check_list({rt(3, 30, 40, 0, 0), rt(3, 45, 50, 12, '+'), rt(3, 20, 25, 12, '-')}, md);   // a lead-in over another target's body
        check_list({rt(3, 30, 40, 4, 0), rt(3, 40, 50, 4, 0), rt(3, 50, 51, 0, 0)}, md);         // touching
        check_list({rt(0, 0, 2, 3, 0), rt(1, 7, 39, 1, '-'), rt(1, 38, 39, 40, '+')}, md);       // a contig of one column
        {
            sfa::ReachPrepared p;
            const std::vector<sfa_reach_target_t> only_minus = {rt(3, 40, 50, 10, '-')};
            sfa::reach_prepare(only_minus.data(), 1, md.m, &p);
            CHECK(p.runs.size() == (strands == 2 ? 2u : 0u));  // a '-' target admits nothing without '-' jobs; else a body and a lead-in
        }
        // ---- random lists: every strand, leads from 0 to beyond the contig ----
        uint32_t state = 12345u + static_cast<uint32_t>(strands);
        const auto rnd = [&](uint32_t n) {
            state = state * 1664525u + 1013904223u;
            return static_cast<int32_t>((state >> 8) % n);
        };
        for (int rep = 0; rep < 60; ++rep) {
            std::vector<sfa_reach_target_t> list;
            const int n = 1 + rnd(12);
            for (int k = 0; k < n; ++k) {
                const int32_t c = rnd(4), limit = offs[c] + lens[c] + 1;
                const int32_t b = rnd(static_cast<uint32_t>(limit)), e = b + 1 + rnd(static_cast<uint32_t>(limit - b));
                const int32_t lead = rnd(3) == 0 ? 0 : rnd(3) == 0 ? rnd(200) : rnd(15);
                list.push_back(rt(c, b, e, lead, "\0+-"[rnd(3)]));
            }
            check_list(list, md);
        }
    }
    printf("selftest ok %d\n", n_cases);
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest")) {
            selftest();
        } else if (!strcmp(word, "reach")) {
            int strands, num_ref, cap, n, n_iv;
            if (scanf("%d %d", &strands, &num_ref) != 2) return 2;
            std::vector<int32_t> lens(num_ref), offs(num_ref);
            for (int r = 0; r < num_ref; ++r)
                if (scanf("%d %d", &lens[r], &offs[r]) != 2) return 2;
            if (scanf("%d %d", &cap, &n) != 2 || n < 0) return 2;
            std::vector<sfa_reach_target_t> t(static_cast<size_t>(n));
            for (sfa_reach_target_t &x : t) {
                char st[8];
                memset(&x, 0, sizeof x);
                if (scanf("%d %d %d %d %7s", &x.contig, &x.begin, &x.end, &x.lead, st) != 5) return 2;
                x.strand = st[0] == '.' ? 0 : static_cast<int8_t>(st[0]);
            }
            if (scanf("%d", &n_iv) != 1 || n_iv < 0) return 2;
            std::vector<sfa_target_t> iv(static_cast<size_t>(n_iv));
            for (sfa_target_t &x : iv)
                if (scanf("%d %d %d", &x.contig, &x.begin, &x.end) != 3) return 2;
            const Model md(lens, offs, strands);
            char msg[224];
            if (const char *why = sfa::reach_list_error(t.data(), n, md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            if (const char *why = sfa::coverage_list_error(iv.data(), n_iv, md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            std::vector<uint32_t> mask, mask2, live, depth(static_cast<size_t>(md.cov_off.back()), 0u);
            std::vector<int32_t> anchor, entry;
            const int64_t on = sfa::reach_tables(t.data(), n, md.m, &mask, &anchor);
            sfa::ReachPrepared p;
            sfa::reach_prepare(t.data(), n, md.m, &p);
            if (sfa::reach_tables_from_runs(p, md.m, &mask2, &entry) != on || mask2 != mask) {
                printf("FAILED the runs give another mask\n");
                return 1;
            }
            sfa::coverage_add(iv.data(), n_iv, md.m, md.cov_off.data(), depth.data());
            const int64_t n_live = sfa::reach_live_mask(mask, entry, depth.data(), md.cov_off.data(), static_cast<uint32_t>(cap), md.m, &live);
            printf("mask %lld", static_cast<long long>(on));
            for (size_t w = 0; w + 1 < mask.size(); ++w) printf(" %08x", mask[w]);
            printf("\nanchor");
            for (const int32_t v : anchor) printf(" %d", v);
            printf("\nentry");
            for (const int32_t v : entry) printf(" %d", v);
            printf("\nlive %lld", static_cast<long long>(n_live));
            for (size_t w = 0; w + 1 < live.size(); ++w) printf(" %08x", live[w]);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
