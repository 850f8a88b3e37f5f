// The host rules of a session's target groups (sigfish_amd/csrc/group_rules.hpp, the header sfa_session_targets.hip builds its label table
// and decides with) as a stand-alone host program, built from that header alone; tests/test_session_groups_cpu.py runs it plain
// and under ASan + UBSan.
//   selftest                      the labels of every case against a loop that calls place_col (row_rules.hpp) for every column
//                                 and every interval; every refusal; the key order; heads; the decision table.
//                                 Prints "selftest ok <cases>".
//   labels <strands> <num_ref> <len, offset per contig> <n_groups> <n> <contig begin end group per target>
//                                 "refused <text>", or "labels <columns in a group> <label per column ...>"
//   decide <best> <second> <best_score> <second_score> <n_events> <valid> <min_events> <margin>
//                                 "decide <index or -1>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "group_rules.hpp"

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

// every column against every interval, through place_col: the lowest group id that covers it, or n_groups
std::vector<uint16_t> brute(const Model &md, const std::vector<sfa_group_target_t> &t, int32_t n_groups) {
    std::vector<uint16_t> label(static_cast<size_t>(md.m.total_cols));
    for (int32_t j = 0; j < md.m.n_jobs; ++j)
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const int32_t r = md.job_contig[j];
            const int x = sfa::place_col(md.job_strand[j], col, md.ref_len[r], md.ref_off[r]);
            int32_t g = n_groups;
            for (const sfa_group_target_t &k : t)
                if (k.contig == r && k.begin <= x && x < k.end && k.group < g) g = k.group;
            label[static_cast<size_t>(md.col_off[j] + col)] = static_cast<uint16_t>(g);
        }
    return label;
}

int n_cases = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

void check_labels(const Model &md, const std::vector<sfa_group_target_t> &t, int32_t n_groups) {
    char msg[256];
    CHECK(sfa::group_list_error(t.data(), static_cast<int32_t>(t.size()), n_groups, md.m, msg, sizeof msg) == nullptr);
    std::vector<uint16_t> got;
    const int64_t in = sfa::group_labels(t.data(), static_cast<int32_t>(t.size()), n_groups, md.m, &got);
    const std::vector<uint16_t> want = brute(md, t, n_groups);
    CHECK(got.size() == 4 * sfa::group_label_words(md.m.total_cols) && got.size() >= want.size() + 4);
    int64_t want_in = 0;
    for (size_t c = 0; c < want.size(); ++c) {
        CHECK(got[c] == want[c]);
        want_in += want[c] != n_groups;
    }
    for (size_t c = want.size(); c < got.size(); ++c) CHECK(got[c] == n_groups);  // the padding is background
    CHECK(in == want_in);
    ++n_cases;
}

void refused(const Model &md, sfa_group_target_t t, int32_t n_groups, const char *word) {
    char msg[256];
    const sfa_group_target_t list[2] = {{0, md.ref_off[0], md.ref_off[0] + 1, 0}, t};  // (the refused one is target 1)
    const char *why = sfa::group_list_error(list, 2, n_groups, md.m, msg, sizeof msg);
    CHECK(why != nullptr && strstr(why, word) != nullptr);
    CHECK(n_groups < 1 || n_groups > sfa::kGroupMax || strncmp(why, "target 1: ", 10) == 0);
    ++n_cases;
}

sfa_group_head_t head(int32_t best, int32_t second, float bs, float ss, int32_t n, int32_t valid = 1) { return sfa_group_head_t{best, second, bs, ss, n, valid}; }

float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

void selftest() {
    const std::vector<int32_t> lens = {1, 31, 32, 33, 64, 65, 300};
    for (int strands = 1; strands <= 2; ++strands)  // 1: RNA, the forward arrays only; 2: DNA
        for (int shift = 0; shift < 2; ++shift) {
            std::vector<int32_t> offs(lens.size(), 0);
            if (shift) offs = {0, 7, 0, 100, 3, 0, 1000};  // ref_st_offset != 0
            const Model md(lens, offs, strands);
            const int32_t o6 = offs[6], o4 = offs[4], o3 = offs[3];
            check_labels(md, {}, 1);  // the empty list: everything background
            for (int32_t r = 0; r < md.m.num_ref; ++r) {
                const int32_t off = offs[r], rl = lens[r];
                check_labels(md, {{r, off, off + rl + 1, 0}}, 1);  // the whole contig; the interval ends at ref_st_offset + ref_length + 1
                check_labels(md, {{r, off + rl, off + rl + 1, 2}}, 3);
                check_labels(md, {{r, off, off + 1, 1}, {r, off + rl - 1 > off ? off + rl - 1 : off, off + rl + 1, 0}}, 2);
            }
            // overlaps of two and of three groups, in either order of the ids: the lowest id wins
            check_labels(md, {{6, o6 + 10, o6 + 60, 1}, {6, o6 + 40, o6 + 90, 0}}, 2);
            check_labels(md, {{6, o6 + 10, o6 + 60, 0}, {6, o6 + 40, o6 + 90, 1}}, 2);
            check_labels(md, {{6, o6 + 10, o6 + 100, 2}, {6, o6 + 30, o6 + 80, 1}, {6, o6 + 50, o6 + 60, 0}, {6, o6 + 55, o6 + 200, 3}}, 4);
            check_labels(md, {{6, o6 + 50, o6 + 60, 3}, {6, o6 + 30, o6 + 80, 2}, {6, o6 + 10, o6 + 100, 1}}, 5);
            // touching intervals of different groups, and of the same group
            check_labels(md, {{4, o4 + 0, o4 + 20, 0}, {4, o4 + 20, o4 + 40, 1}, {4, o4 + 40, o4 + 65, 0}}, 2);
            // an empty group (1 has no interval; 3 has one that covers no column: coordinates below the offset)
            check_labels(md, {{3, o3 + 1, o3 + 9, 0}, {3, o3 + 5, o3 + 30, 2}}, 3);
            if (shift) check_labels(md, {{3, 0, 100, 3}, {6, 5, 1000, 3}, {3, o3 + 1, o3 + 9, 0}}, 4);
            // unsorted, on several contigs, the largest id and the largest n_groups
            check_labels(md, {{6, o6 + 200, o6 + 260, 1022}, {6, o6 + 10, o6 + 40, 5}, {3, o3 + 5, o3 + 20, 700}, {1, offs[1], offs[1] + 32, 0}, {6, o6 + 30, o6 + 64, 4}}, 1023);
            // every column its own group
            {
                std::vector<sfa_group_target_t> each;
                for (int32_t c = 0; c < 64; ++c) each.push_back({4, o4 + c, o4 + c + 1, 63 - c});
                check_labels(md, each, 64);
            }
            // every refusal: target_list_error's, a bad group id, a bad n_groups
            refused(md, {-1, 0, 1, 0}, 2, "contig");
            refused(md, {7, 0, 1, 0}, 2, "contig");
            refused(md, {2, -1, 4, 0}, 2, "negative");
            refused(md, {2, 4, 4, 0}, 2, "empty");
            refused(md, {2, 5, 4, 0}, 2, "empty");
            refused(md, {2, 0, offs[2] + 32 + 2, 0}, 2, "beyond");
            refused(md, {2, 0, 4, -1}, 2, "group");
            refused(md, {2, 0, 4, 2}, 2, "group");
            refused(md, {2, 0, 4, 0}, 0, "n_groups");
            refused(md, {2, 0, 4, 0}, -3, "n_groups");
            refused(md, {2, 0, 4, 0}, 1024, "n_groups");
        }
    // the key order on {0, denormal, 1, 3e38, +inf} x columns: the u64 order is (cost, column) lexicographic, i.e. class_before
    {
        const float costs[] = {0.0f, from_bits(1u), from_bits(0x007fffffu), 1.0f, 3e38f, INFINITY};
        const int32_t cols[] = {0, 1, 2, 8191, 8192, 1 << 20, INT32_MAX - 1};
        for (const float ca : costs)
            for (const int32_t ga : cols)
                for (const float cb : costs)
                    for (const int32_t gb : cols) {
                        const uint64_t ka = sfa::group_key(ca, ga), kb = sfa::group_key(cb, gb);
                        CHECK((ka < kb) == sfa::class_before(ca, ga, cb, gb) && (ka == kb) == (ca == cb && ga == gb));
                        CHECK(ka != sfa::kGroupNoKey && ka < sfa::kGroupNoKey);
                        CHECK(sfa::group_key_col(ka) == ga);
                        const float back = sfa::group_key_cost(ka);
                        CHECK(memcmp(&back, &ca, 4) == 0);
                        ++n_cases;
                    }
        CHECK(sfa::group_key_col(sfa::kGroupNoKey) == sfa::kNoColumn && std::isinf(sfa::group_key_cost(sfa::kGroupNoKey)));
    }
    // heads: the two smallest keys, whichever way they are merged
    {
        const uint64_t none = sfa::kGroupNoKey;
        const uint64_t keys[6] = {sfa::group_key(5.f, 40), none, sfa::group_key(2.f, 90), sfa::group_key(2.f, 7), none, sfa::group_key(INFINITY, 3)};
        sfa_group_head_t h = sfa::group_head(keys, 6);
        CHECK(h.best == 3 && h.second == 2 && h.best_score == 2.f && h.second_score == 2.f && h.valid == 1);
        h = sfa::group_head(keys, 2);
        CHECK(h.best == 0 && h.second == -1 && h.best_score == 5.f && std::isinf(h.second_score));
        h = sfa::group_head(keys + 4, 2);
        CHECK(h.best == 1 && h.second == -1 && std::isinf(h.best_score));
        h = sfa::group_head(keys + 4, 1);
        CHECK(h.best == -1 && h.second == -1 && std::isinf(h.best_score) && std::isinf(h.second_score));
        for (int split = 0; split <= 6; ++split) {  // pairwise merge of disjoint halves equals the scan
            sfa::GroupTop2 a = sfa::group_top2_none(), b = sfa::group_top2_none();
            for (int e = 0; e < 6; ++e) sfa::group_top2_offer(e < split ? a : b, keys[e], e);
            for (int way = 0; way < 2; ++way) {
                const sfa::GroupTop2 m = way ? sfa::group_top2_merge(b, a) : sfa::group_top2_merge(a, b);
                CHECK(m.e1 == 3 && m.e2 == 2 && m.k1 == keys[3] && m.k2 == keys[2]);
                ++n_cases;
            }
        }
        const sfa_group_head_t off = sfa::group_head_none();
        CHECK(off.valid == 0 && off.best == -1 && off.second == -1 && std::isinf(off.best_score) && std::isinf(off.second_score) && off.n_events == 0);
    }
    // the decision table
    const float inf = INFINITY;
    struct Row {
        sfa_group_head_t h;
        int min_events;
        float margin;
        int want;
    };
    const Row table[] = {
        {head(3, 1, 10.f, 60.f, 100), 100, 0.5f, 3},       // margin exactly met (50 = 0.5 * 100), n at min_events
        {head(3, 1, 10.f, 59.5f, 100), 100, 0.5f, -1},     // margin just missed
        {head(3, 1, 10.f, 60.f, 99), 100, 0.5f, -1},       // n_events < min_events
        {head(7, -1, 10.f, inf, 100), 100, 1e30f, 7},      // an empty runner-up counts as +inf: any finite margin
        {head(7, -1, 10.f, 3.f, 100), 100, 0.5f, 7},       // ... whatever its score field holds
        {head(2, 5, 10.f, inf, 100), 100, 1e30f, 2},       // a runner-up whose every column costs +inf
        {head(2, 5, inf, inf, 100), 100, 0.f, -1},         // both +inf: nothing to tell apart
        {head(-1, -1, inf, inf, 100), 100, 0.f, -1},       // no entry has a column
        {head(3, 1, 10.f, 60.f, 100, 0), 100, 0.5f, -1},   // valid = 0
        {head(3, 1, 10.f, 60.f, 100), 100, -1.f, -1},      // a negative margin
        {head(3, 1, 10.f, 60.f, 100), 100, inf, -1},       // a margin that is not finite
        {head(3, 1, 10.f, 60.f, 100), 100, NAN, -1},
        {head(1023, 0, 10.f, 10.f, 100), 100, 0.f, 1023},  // margin 0 and equal scores: the background, which holds the lower column
        {head(0, 1, 10.f, 60.f, 0), 0, 0.5f, 0},           // min_events 0
    };
    for (const Row &r : table) {
        CHECK(sfa::group_decide(r.h, r.min_events, r.margin) == r.want);
        ++n_cases;
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
            int strands, num_ref, n, n_groups;
            if (scanf("%d %d", &strands, &num_ref) != 2 || num_ref < 1 || num_ref > 4096) return 2;
            std::vector<int32_t> lens(num_ref), offs(num_ref);
            for (int r = 0; r < num_ref; ++r)
                if (scanf("%d %d", &lens[r], &offs[r]) != 2) return 2;
            if (scanf("%d %d", &n_groups, &n) != 2 || n < 0 || n > 1 << 20) return 2;
            std::vector<sfa_group_target_t> t(n);
            for (int k = 0; k < n; ++k)
                if (scanf("%d %d %d %d", &t[k].contig, &t[k].begin, &t[k].end, &t[k].group) != 4) return 2;
            const Model md(lens, offs, strands);
            char msg[256];
            if (const char *why = sfa::group_list_error(t.data(), n, n_groups, md.m, msg, sizeof msg)) {
                printf("refused %s\n", why);
                continue;
            }
            std::vector<uint16_t> label;
            const int64_t in = sfa::group_labels(t.data(), n, n_groups, md.m, &label);
            printf("labels %lld", static_cast<long long>(in));
            for (int64_t c = 0; c < md.m.total_cols; ++c) printf(" %d", label[static_cast<size_t>(c)]);
            printf("\n");
        } else if (!strcmp(word, "decide")) {
            int best, second, n, valid, min_events;
            float bs, ss, margin;
            if (scanf("%d %d %f %f %d %d %d %f", &best, &second, &bs, &ss, &n, &valid, &min_events, &margin) != 8) return 2;
            printf("decide %d\n", sfa::group_decide(head(best, second, bs, ss, n, valid), min_events, margin));
        } else {
            return 2;
        }
    }
    return 0;
}
