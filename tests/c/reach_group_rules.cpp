// The host rules of a session's reach groups (sigfish_amd/csrc/reach_group_rules.hpp, the header sfa_session_targets.hip and the kernels of
// sdtw_session_reachgroup.hpp share) as a stand-alone host program, built from that header alone;
// tests/test_reach_group_rules_cpu.py runs it plain and under ASan + UBSan.
//   selftest      the list refusals; reach_group_tables against a second, brute-force statement (per column over every target, the
//                 admitting set and each target's own anchor spelled out); the prepared runs -- rising, disjoint, inside the job --
//                 bisected on the host equal to the tables; the three consequences of the rule (group_labels at lead 0 and strand
//                 0, reach_tables' anchors with the groups dropped, a label is a group exactly where reach_tables sets the mask
//                 bit); a body never loses its label to another group's lead-in; the live rule and the records' body columns
//                 against per-column statements; the named cases; a few thousand random lists.  Prints "selftest ok <cases>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "reach_group_rules.hpp"

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

typedef sfa_reach_group_target_t RG;

RG rg(int32_t contig, int32_t begin, int32_t end, int32_t lead, int32_t group, int strand) {
    RG t{};
    t.contig = contig, t.begin = begin, t.end = end, t.lead = lead, t.group = group, t.strand = static_cast<int8_t>(strand);
    return t;
}

// the second statement: per column the admitting targets with their own anchors, from the two inequalities, in 64 bits; the label
// is the lowest group among those whose anchor is the best one
void brute(const std::vector<RG> &t, int32_t n_groups, const Model &md, std::vector<uint16_t> *label, std::vector<int32_t> *anchor) {
    label->assign(4 * sfa::group_label_words(md.m.total_cols), static_cast<uint16_t>(n_groups));
    anchor->assign(static_cast<size_t>(md.m.total_cols), -1);
    for (int32_t j = 0; j < md.m.n_jobs; ++j) {
        const int32_t c = md.job_contig[j], rl = md.ref_len[c], off = md.ref_off[c];
        const bool plus = md.job_strand[j] == '+';
        for (int32_t col = 0; col < rl; ++col) {
            const long long x = plus ? static_cast<long long>(col) + off : static_cast<long long>(rl) - col + off;
            std::vector<long long> cand;
            std::vector<int32_t> group;
            for (const RG &q : t) {
                if (q.contig != c) continue;
                if (q.strand == '+' && !plus) continue;
                if (q.strand == '-' && plus) continue;
                const long long b = q.begin, e = q.end, l = q.lead;
                if (plus && b - l <= x && x < e) cand.push_back(x > b ? x : b), group.push_back(q.group);
                if (!plus && b <= x && x < e + l) cand.push_back(x < e - 1 ? x : e - 1), group.push_back(q.group);
            }
            if (cand.empty()) continue;
            long long best = cand[0];
            for (const long long v : cand) best = plus ? (v < best ? v : best) : (v > best ? v : best);
            int32_t g = n_groups;
            for (size_t k = 0; k < cand.size(); ++k)
                if (cand[k] == best && group[k] < g) g = group[k];
            const size_t at = static_cast<size_t>(md.col_off[j] + col);
            (*label)[at] = static_cast<uint16_t>(g);
            (*anchor)[at] = static_cast<int32_t>(best);
        }
    }
}

struct Tables {
    std::vector<uint16_t> label;
    std::vector<int32_t> anchor, entry;
};

// everything that holds for every list
Tables check_list(const std::vector<RG> &t, int32_t n_groups, const Model &md) {
    const int32_t n = static_cast<int32_t>(t.size());
    char msg[256];
    CHECK(sfa::reach_group_list_error(t.data(), n, n_groups, md.m, msg, sizeof msg) == nullptr);
    Tables T;
    std::vector<uint16_t> label2, label3;
    std::vector<int32_t> anchor2;
    const int64_t in = sfa::reach_group_tables(t.data(), n, n_groups, md.m, &T.label, &T.anchor);
    brute(t, n_groups, md, &label2, &anchor2);
    CHECK(T.label == label2);
    CHECK(T.anchor == anchor2);
    // the prepared runs: rising, disjoint, inside the job, labels in range; bisected they give the model's tables
    sfa::ReachGroupPrepared p;
    sfa::reach_group_prepare(t.data(), n, md.m, &p);
    CHECK(sfa::reach_group_tables_from_runs(p, n_groups, md.m, &label3, &T.entry) == in);
    CHECK(label3 == T.label);
    for (int32_t j = 0; j < md.m.n_jobs; ++j) {
        const int32_t c = md.job_contig[j];
        for (int32_t r = p.run_off[j]; r < p.run_off[j + 1]; ++r) {
            if (!(p.runs[r].lo < p.runs[r].hi && p.runs[r].lo >= 0 && p.runs[r].hi <= md.job_len[j])) CHECK(false);
            if (!(p.runs[r].label >= 0 && p.runs[r].label < n_groups)) CHECK(false);
            if (r > p.run_off[j] && !(p.runs[r - 1].hi <= p.runs[r].lo)) CHECK(false);
        }
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const size_t g = static_cast<size_t>(md.col_off[j] + col);
            if (T.entry[g] != sfa::reach_entry_of(T.anchor[g], md.ref_off[c])) CHECK(false);
            if (T.entry[g] >= 0 && T.entry[g] > md.ref_len[c]) CHECK(false);  // inside the contig's track
        }
    }
    for (size_t g = static_cast<size_t>(md.m.total_cols); g < T.label.size(); ++g)
        if (T.label[g] != n_groups) CHECK(false);  // the padding holds the background
    // consequence 2 and 3: reach_tables' anchors of the list with the groups dropped; a label is a group exactly where the mask bit is set
    const std::vector<sfa_reach_target_t> reach = sfa::reach_group_reach_list(t.data(), n);
    std::vector<uint32_t> mask;
    std::vector<int32_t> ranchor;
    CHECK(sfa::reach_tables(reach.data(), n, md.m, &mask, &ranchor) == in);
    CHECK(ranchor == T.anchor);
    for (int64_t g = 0; g < md.m.total_cols; ++g)
        if (((mask[static_cast<size_t>(g >> 5)] >> (g & 31)) & 1u) != (T.label[static_cast<size_t>(g)] != n_groups)) CHECK(false);
    // the anchors of reach_prepare's runs are these runs' (the prepared forms agree, column by column)
    {
        sfa::ReachPrepared rp;
        std::vector<uint32_t> mask2;
        std::vector<int32_t> rentry;
        sfa::reach_prepare(reach.data(), n, md.m, &rp);
        sfa::reach_tables_from_runs(rp, md.m, &mask2, &rentry);
        CHECK(rentry == T.entry);
    }
    // consequence 4: inside a body the label is the lowest group among the BODIES over the column, whatever lead-ins cross it
    for (int32_t j = 0; j < md.m.n_jobs; ++j) {
        const int32_t c = md.job_contig[j];
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const int32_t x = sfa::place_col(md.job_strand[j], col, md.ref_len[c], md.ref_off[c]);
            int32_t g = n_groups;
            for (const RG &q : t)
                if (q.contig == c && (q.strand == 0 || q.strand == md.job_strand[j]) && q.begin <= x && x < q.end && q.group < g) g = q.group;
            if (g != n_groups && T.label[static_cast<size_t>(md.col_off[j] + col)] != g) CHECK(false);
        }
    }
    // consequence 1: every lead 0 and every strand 0: group_labels bit for bit
    bool plain = true;
    for (const RG &q : t) plain = plain && q.lead == 0 && q.strand == 0;
    if (plain) {
        std::vector<sfa_group_target_t> gt;
        for (const RG &q : t) gt.push_back(sfa_group_target_t{q.contig, q.begin, q.end, q.group});
        std::vector<uint16_t> want;
        CHECK(sfa::group_labels(gt.data(), n, n_groups, md.m, &want) == in);
        CHECK(want == T.label);
    }
    ++n_cases;
    return T;
}

// the live table and the records under a depth, against per-column statements
void check_depth(const Tables &T, const std::vector<sfa_target_t> &iv, uint32_t cap, int32_t n_groups, const Model &md) {
    std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off.back()), 0u);
    sfa::coverage_add(iv.data(), static_cast<int32_t>(iv.size()), md.m, md.cov_off.data(), depth.data());
    std::vector<uint16_t> live;
    std::vector<int32_t> first;
    std::vector<sfa_group_cover_t> rec, want(static_cast<size_t>(n_groups) + 1, sfa::group_cover_none());
    const int64_t in = sfa::reach_group_live_labels(T.label, T.entry, depth.data(), md.cov_off.data(), cap, n_groups, md.m, &live, &first);
    sfa::reach_group_records(T.label, T.entry, depth.data(), md.cov_off.data(), cap, n_groups, md.m, &rec);
    int64_t in2 = 0;
    std::vector<int32_t> first2(static_cast<size_t>(n_groups) + 1, sfa::kNoColumn);
    for (int32_t j = 0; j < md.m.n_jobs; ++j) {
        const int32_t c = md.job_contig[j], off = md.ref_off[c];
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const size_t g = static_cast<size_t>(md.col_off[j] + col);
            // the depth of the anchor COORDINATE (0 below the track), not of the column's own
            const int32_t a = T.anchor[g];
            const uint32_t d = (a < 0 || a < off) ? 0u : depth[static_cast<size_t>(md.cov_off[c] + a - off)];
            const uint16_t l = (T.label[g] != n_groups && d < cap) ? T.label[g] : static_cast<uint16_t>(n_groups);
            if (live[g] != l) CHECK(false);
            in2 += l != n_groups;
            if (first2[l] == sfa::kNoColumn) first2[l] = static_cast<int32_t>(g);
            const int32_t x = sfa::place_col(md.job_strand[j], col, md.ref_len[c], off);
            if (md.job_strand[j] == '+' && a == x) sfa::group_cover_note(want[T.label[g]], depth[static_cast<size_t>(md.cov_off[c] + x - off)], cap);
        }
    }
    CHECK(in == in2);
    CHECK(first == first2);
    for (size_t e = 0; e < rec.size(); ++e)
        if (memcmp(&rec[e], &want[e], sizeof rec[e]) != 0) CHECK(false);
    ++n_cases;
}

uint16_t label_at(const Tables &T, const Model &md, int32_t job, int32_t x) {  // the label of the column of `job` that reports coordinate x
    const int32_t c = md.job_contig[job];
    for (int32_t col = 0; col < md.job_len[job]; ++col)
        if (sfa::place_col(md.job_strand[job], col, md.ref_len[c], md.ref_off[c]) == x) return T.label[static_cast<size_t>(md.col_off[job] + col)];
    CHECK(false);
    return 0;
}
int32_t entry_at(const Tables &T, const Model &md, int32_t job, int32_t x) {
    const int32_t c = md.job_contig[job];
    for (int32_t col = 0; col < md.job_len[job]; ++col)
        if (sfa::place_col(md.job_strand[job], col, md.ref_len[c], md.ref_off[c]) == x) return T.entry[static_cast<size_t>(md.col_off[job] + col)];
    CHECK(false);
    return 0;
}

void selftest() {
    const std::vector<int32_t> lens = {1, 31, 33, 70}, offs = {0, 7, 100, 3};
    for (int strands = 1; strands <= 2; ++strands) {
        const Model md(lens, offs, strands);
        char msg[256], want[256];
        // ---- the refusals: reach_list_error's, with its words; group_list_error's for group ids and n_groups ----
        {
            const sfa_reach_target_t bad[] = {{-1, 0, 1, 0, 0, {0, 0, 0}},  {4, 0, 1, 0, 0, {0, 0, 0}},          {2, -1, 4, 0, 0, {0, 0, 0}},
                                              {2, 4, 4, 0, 0, {0, 0, 0}},   {2, 0, 136, 0, 0, {0, 0, 0}},        {2, 100, 110, -1, 0, {0, 0, 0}},
                                              {2, 100, 110, (1 << 30) + 1, 0, {0, 0, 0}}, {2, 100, 110, 0, 'x', {0, 0, 0}}, {2, 100, 110, 0, '-', {0, 1, 0}}};
            for (const sfa_reach_target_t &b : bad) {
                const sfa_reach_target_t two[] = {{2, 100, 110, 5, '+', {0, 0, 0}}, b};
                CHECK(sfa::reach_list_error(two, 2, md.m, want, sizeof want) != nullptr);
                RG list[] = {rg(2, 100, 110, 5, 0, '+'), rg(b.contig, b.begin, b.end, b.lead, 1, b.strand)};
                memcpy(list[1].pad, b.pad, 3);
                const char *why = sfa::reach_group_list_error(list, 2, 2, md.m, msg, sizeof msg);
                CHECK(why != nullptr && !strcmp(why, want));
            }
            for (const int32_t ng : {0, -1, sfa::kGroupMax + 1}) {
                CHECK(sfa::group_list_error(nullptr, 0, ng, md.m, want, sizeof want) != nullptr);
                const RG x = rg(2, 100, 110, 5, 0, 0);
                const char *why = sfa::reach_group_list_error(&x, 1, ng, md.m, msg, sizeof msg);
                CHECK(why != nullptr && !strcmp(why, want));
            }
            for (const int32_t g : {-1, 3, 1 << 20}) {
                const sfa_group_target_t two[] = {{2, 100, 110, 0}, {3, 10, 20, g}};
                CHECK(sfa::group_list_error(two, 2, 3, md.m, want, sizeof want) != nullptr);
                const RG list[] = {rg(2, 100, 110, 9, 0, '-'), rg(3, 10, 20, 4, g, 0)};
                const char *why = sfa::reach_group_list_error(list, 2, 3, md.m, msg, sizeof msg);
                CHECK(why != nullptr && !strcmp(why, want));
            }
            CHECK(strstr(sfa::reach_group_list_error(nullptr, sfa::kReachTargetsMax + 1, 4, md.m, msg, sizeof msg), "at most") != nullptr);  // the count comes first
            CHECK(sfa::reach_group_list_error(nullptr, 0, 1, md.m, msg, sizeof msg) == nullptr);
        }
        // ---- the named cases ----
        const int32_t jp = 3 * strands, jm = 3 * strands + 1;  // contig 3's jobs ('-' only with two strands)
        {  // two targets with equal begin and different groups: the lead-in and the shared body go to the lower id, the rest of the longer body to its own
            const Tables T = check_list({rg(3, 40, 50, 10, 5, '+'), rg(3, 40, 45, 10, 2, '+')}, 8, md);
            CHECK(label_at(T, md, jp, 35) == 2 && label_at(T, md, jp, 40) == 2 && label_at(T, md, jp, 44) == 2 && label_at(T, md, jp, 45) == 5 && label_at(T, md, jp, 29) == 8);
            const Tables U = check_list({rg(3, 40, 45, 10, 2, '+'), rg(3, 40, 50, 10, 5, '+')}, 8, md);  // (in either list order)
            CHECK(U.label == T.label);
            if (strands == 2) {  // on '-' the two share no first base: 49 is group 5's alone, the lead-in beyond 50 leads to it
                const Tables V = check_list({rg(3, 40, 50, 10, 5, 0), rg(3, 40, 45, 10, 2, 0)}, 8, md);
                CHECK(label_at(V, md, jm, 55) == 5 && label_at(V, md, jm, 49) == 5 && label_at(V, md, jm, 44) == 2 && label_at(V, md, jm, 45) == 5);
            }
        }
        {  // a body inside another group's lead-in: the body keeps its label, in front of it the nearer body wins, behind it the lead-in goes on
            const Tables T = check_list({rg(3, 50, 60, 30, 0, '+'), rg(3, 30, 35, 0, 1, '+')}, 2, md);
            CHECK(label_at(T, md, jp, 29) == 0 && label_at(T, md, jp, 30) == 1 && label_at(T, md, jp, 34) == 1 && label_at(T, md, jp, 35) == 0 && label_at(T, md, jp, 19) == 2);
            CHECK(entry_at(T, md, jp, 29) == 50 - 3 && entry_at(T, md, jp, 32) == 32 - 3);
            const Tables U = check_list({rg(3, 50, 60, 30, 0, '+'), rg(3, 30, 35, 3, 1, '+')}, 2, md);  // with a lead of its own: nearer, so it takes 27 .. 29
            CHECK(label_at(U, md, jp, 26) == 0 && label_at(U, md, jp, 27) == 1 && label_at(U, md, jp, 35) == 0);
        }
        {  // a lead clipped at the contig's first column
            const Tables T = check_list({rg(3, 8, 12, 400, 4, '+')}, 5, md);
            CHECK(label_at(T, md, jp, 3) == 4 && entry_at(T, md, jp, 3) == 8 - 3 && T.label[static_cast<size_t>(md.col_off[jp])] == 4);
        }
        if (strands == 2) {  // a '-' target ending at or below ref_st_offset: kReachBelowTrack
            const int32_t j2 = 2 * strands + 1;
            const Tables T = check_list({rg(2, 0, 100, 20, 1, '-'), rg(2, 0, 101, 3, 0, '-')}, 2, md);
            CHECK(entry_at(T, md, j2, 101) == 0 && label_at(T, md, j2, 101) == 0);      // the second's lead-in (a '-' row reports 101 .. 133): anchor 100, entry 0
            CHECK(entry_at(T, md, j2, 103) == 0 && label_at(T, md, j2, 104) == 1);      // ... up to 103; from 104 on only the first reaches
            CHECK(entry_at(T, md, j2, 105) == sfa::kReachBelowTrack && label_at(T, md, j2, 105) == 1);  // only the first reaches: anchor 99, below the track
            check_depth(T, {{2, 100, 101}, {2, 100, 101}}, 1, 2, md);
            std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off.back()), 7u);
            CHECK(sfa::reach_group_live_label(1, depth.data(), sfa::kReachBelowTrack, 34, 1, 2) == 1);  // depth 0 by definition
        }
        for (const int32_t ng : {1, sfa::kGroupMax}) {  // n_groups of 1 and of 1023
            const Tables T = check_list({rg(3, 40, 50, 10, ng - 1, 0), rg(1, 10, 12, 2, 0, '+')}, ng, md);
            CHECK(label_at(T, md, jp, 33) == ng - 1 && label_at(T, md, jp, 29) == ng);
            check_depth(T, {{3, 40, 41}}, 1, ng, md);
        }
        {  // the live rule at depths cap - 1 and cap, read at the ANCHOR
            const uint32_t track[] = {0, 2, 3, 9};
            CHECK(sfa::reach_group_live_label(1, track, 1, 4, 3, 5) == 1);  // depth 2 = cap - 1
            CHECK(sfa::reach_group_live_label(1, track, 2, 4, 3, 5) == 5);  // depth 3 = cap
            CHECK(sfa::reach_group_live_label(5, track, 0, 4, 3, 5) == 5);  // the background stays
            const Tables T = check_list({rg(3, 40, 50, 10, 0, '+'), rg(3, 60, 65, 5, 1, 0)}, 2, md);
            check_depth(T, {{3, 40, 41}, {3, 40, 41}}, 2, 2, md);            // the body's first base at the cap: the lead-in closes, the rest of the body stays
            check_depth(T, {{3, 40, 41}}, 2, 2, md);                          // at cap - 1: nothing closes
            check_depth(T, {{3, 30, 40}, {3, 30, 40}, {3, 30, 40}}, 2, 2, md);  // the lead-in covered, not the body: nothing closes
            std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off.back()), 0u);
            const sfa_target_t first_base[] = {{3, 40, 41}, {3, 40, 41}}, lead_only[] = {{3, 30, 40}, {3, 30, 40}, {3, 30, 40}};
            std::vector<uint16_t> live;
            std::vector<int32_t> first;
            sfa::coverage_add(first_base, 2, md.m, md.cov_off.data(), depth.data());
            sfa::reach_group_live_labels(T.label, T.entry, depth.data(), md.cov_off.data(), 2, 2, md.m, &live, &first);
            Tables L = T;
            L.label = live;
            CHECK(label_at(L, md, jp, 35) == 2 && label_at(L, md, jp, 40) == 2 && label_at(L, md, jp, 41) == 0 && label_at(L, md, jp, 49) == 0 && label_at(L, md, jp, 57) == 1);
            std::fill(depth.begin(), depth.end(), 0u);
            sfa::coverage_add(lead_only, 3, md.m, md.cov_off.data(), depth.data());
            sfa::reach_group_live_labels(T.label, T.entry, depth.data(), md.cov_off.data(), 2, 2, md.m, &live, &first);
            CHECK(live == T.label);
        }
        {  // the records: body columns of '+' jobs only; a group with '-' targets only has an empty record, and so has the background
            const Tables T = check_list({rg(3, 40, 50, 10, 0, '+'), rg(3, 20, 25, 10, 1, '-')}, 2, md);
            std::vector<uint32_t> depth(static_cast<size_t>(md.cov_off.back()), 1u);
            std::vector<sfa_group_cover_t> rec;
            sfa::reach_group_records(T.label, T.entry, depth.data(), md.cov_off.data(), 1, 2, md.m, &rec);
            CHECK(rec[0].columns == 10 && rec[0].capped == 10 && rec[0].depth_sum == 10 && rec[1].columns == 0 && rec[1].depth_min == UINT32_MAX && rec[2].columns == 0);
        }
        check_list({}, 3, md);
        check_list({rg(3, 30, 40, 4, 0, 0), rg(3, 40, 50, 4, 1, 0), rg(3, 50, 51, 0, 0, 0)}, 2, md);  // touching
        check_list({rg(3, 30, 35, 20, 3, '+'), rg(3, 40, 45, 25, 1, '+'), rg(3, 40, 42, 1, 0, '-')}, 4, md);
        check_list({rg(0, 0, 2, 3, 1, 0), rg(1, 7, 39, 1, 0, '-'), rg(1, 38, 39, 40, 2, '+')}, 3, md);  // a contig of one column
    }
    // ---- random lists: 1-3 contigs of 5-300 k-mers, DNA and RNA, 0-40 targets, leads 0-400, all three strand values ----
    uint32_t state = 2463534242u;
    const auto rnd = [&](uint32_t n) {
        state = state * 1664525u + 1013904223u;
        return static_cast<int32_t>((state >> 8) % n);
    };
    for (int rep = 0; rep < 3000; ++rep) {
        const int num_ref = 1 + rnd(3), strands = 1 + rnd(2);
        std::vector<int32_t> lens, offs;
        for (int r = 0; r < num_ref; ++r) lens.push_back(5 + rnd(296)), offs.push_back(rnd(3) == 0 ? 0 : rnd(40));
        const Model md(lens, offs, strands);
        const int32_t n_groups = rnd(8) == 0 ? sfa::kGroupMax : 1 + rnd(6);
        const bool plain = rnd(10) == 0;  // every lead 0, every strand 0: group_labels
        std::vector<RG> list;
        const int n = rnd(41);
        for (int k = 0; k < n; ++k) {
            const int32_t c = rnd(static_cast<uint32_t>(num_ref)), limit = offs[c] + lens[c] + 1;
            const int32_t b = rnd(static_cast<uint32_t>(limit)), e = b + 1 + rnd(static_cast<uint32_t>(std::min(limit - b, 1 + rnd(60))));
            const int32_t lead = plain || rnd(4) == 0 ? 0 : rnd(3) == 0 ? rnd(401) : rnd(20);
            list.push_back(rg(c, b, e, lead, rnd(static_cast<uint32_t>(n_groups)), plain ? 0 : "\0+-"[rnd(3)]));
        }
        const Tables T = check_list(list, n_groups, md);
        std::vector<sfa_target_t> iv;
        for (int k = rnd(6); k > 0; --k) {
            const int32_t c = rnd(static_cast<uint32_t>(num_ref)), limit = offs[c] + lens[c] + 1;
            const int32_t b = rnd(static_cast<uint32_t>(limit));
            iv.push_back(sfa_target_t{c, b, b + 1 + rnd(static_cast<uint32_t>(limit - b))});
        }
        check_depth(T, iv, static_cast<uint32_t>(1 + rnd(3)), n_groups, md);
    }
    printf("selftest ok %d\n", n_cases);
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest"))
            selftest();
        else
            return 2;
    }
    return 0;
}
