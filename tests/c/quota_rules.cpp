// The host rules of a session's open and closed groups (sigfish_amd/csrc/quota_rules.hpp, the header sfa_session_targets.hip normalises
// the bitmap with and the rows kernel builds its record with) as a stand-alone host program, built from that header alone;
// tests/test_session_quota_cpu.py runs it plain and under ASan + UBSan.
//   selftest      the record of every case against a per-column brute force (place_col of row_rules.hpp for every column and
//                 interval, the caller's own bitmap bit by bit, an explicit (cost, column) comparison); bitmaps at n_groups 1, 31,
//                 32, 33, 64, 65, 1023; set bits at or above n_groups; the tie rule against class_before; the lowest columns of
//                 the classes; the quota book.  Prints "selftest ok <cases>".
//   record <strands> <num_ref> <len, offset per contig> <n_groups> <n> <contig begin end group per target> <n_words, -1: null>
//          <words in hex> <the row's costs as hex bit patterns>
//                 "record <on bits> <off bits> <on_rid> <on_pos_end> <off_rid> <off_pos_end> <on_strand> <off_strand> <on_group>
//                 <off_group> <first_on> <first_off>"
//   book <n_groups> <quota> <n> <group per accepted read>
//                 "book <1 / 0 per read: the bitmap changed> | <accepted per group> | <words in hex>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "quota_rules.hpp"

namespace {

struct Model {
    std::vector<int32_t> job_contig, job_len, ref_len, ref_off;
    std::vector<int8_t> job_strand;
    std::vector<int64_t> col_off;
    sfa::TargetModel m;
    sfa::RefTables ref;
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
        ref = sfa::RefTables{job_contig.data(), job_strand.data(), ref_len.data(), ref_off.data()};
    }
};

int n_cases = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

struct Want {
    float c[2];
    int32_t rid[2], pos[2], strand[2], group[2], col[2];
};

// column by column, nothing of quota_rules.hpp or group_labels: the label through place_col, the class from the caller's words
Want brute(const Model &md, const std::vector<sfa_group_target_t> &t, int32_t n_groups, const uint32_t *open, const std::vector<float> &row) {
    Want w;
    for (int k = 0; k < 2; ++k) w.c[k] = INFINITY, w.rid[k] = w.pos[k] = w.group[k] = w.col[k] = -1, w.strand[k] = 0;
    for (int32_t j = 0; j < md.m.n_jobs; ++j)
        for (int32_t col = 0; col < md.job_len[j]; ++col) {
            const int32_t r = md.job_contig[j];
            const int x = sfa::place_col(md.job_strand[j], col, md.ref_len[r], md.ref_off[r]);
            int32_t g = n_groups;
            for (const sfa_group_target_t &q : t)
                if (q.contig == r && q.begin <= x && x < q.end && q.group < g) g = q.group;
            const bool on = g < n_groups && (!open || ((open[g / 32] >> (g % 32)) & 1u));
            const int k = on ? 0 : 1;
            const float c = row[static_cast<size_t>(md.col_off[j] + col)];
            if (w.col[k] < 0 || c < w.c[k]) {  // (columns come in rising order: the first of equal costs stays)
                w.c[k] = c, w.rid[k] = r, w.pos[k] = x, w.strand[k] = md.job_strand[j], w.group[k] = g, w.col[k] = static_cast<int32_t>(md.col_off[j] + col);
            }
        }
    return w;
}

uint32_t rng_state = 12345;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

std::vector<float> random_row(int64_t n, int levels) {  // few levels: ties everywhere
    std::vector<float> row(static_cast<size_t>(n));
    for (float &c : row) c = 1.0f + 0.25f * static_cast<float>(rnd() % levels);
    return row;
}

sfa_open_class_t record_of(const Model &md, const std::vector<sfa_group_target_t> &t, int32_t n_groups, const uint32_t *open, const std::vector<float> &row, int32_t *first_on = nullptr,
                           int32_t *first_off = nullptr) {
    char msg[256];
    CHECK(sfa::group_list_error(t.data(), static_cast<int32_t>(t.size()), n_groups, md.m, msg, sizeof msg) == nullptr);
    std::vector<uint16_t> label;
    sfa::group_labels(t.data(), static_cast<int32_t>(t.size()), n_groups, md.m, &label);
    if (first_on) {
        uint32_t norm[sfa::kOpenWords];
        sfa::open_normalise(open, n_groups, norm);
        std::vector<int32_t> first;
        sfa::open_label_firsts(label.data(), md.m.total_cols, n_groups, &first);
        sfa::open_first_cols(first, n_groups, norm, first_on, first_off);
    }
    return sfa::open_class_of_row(row.data(), label.data(), md.m.total_cols, n_groups, open, md.m.n_jobs, md.col_off.data(), md.ref);
}

void check_record(const Model &md, const std::vector<sfa_group_target_t> &t, int32_t n_groups, const uint32_t *open, const std::vector<float> &row) {
    int32_t first_on, first_off;
    const sfa_open_class_t got = record_of(md, t, n_groups, open, row, &first_on, &first_off);
    const Want w = brute(md, t, n_groups, open, row);
    CHECK(memcmp(&got.cls.on_score, &w.c[0], 4) == 0 && memcmp(&got.cls.off_score, &w.c[1], 4) == 0);
    CHECK(got.cls.on_rid == w.rid[0] && got.cls.on_pos_end == w.pos[0] && got.cls.on_strand == w.strand[0] && got.on_group == w.group[0]);
    CHECK(got.cls.off_rid == w.rid[1] && got.cls.off_pos_end == w.pos[1] && got.cls.off_strand == w.strand[1] && got.off_group == w.group[1]);
    CHECK(got.cls.valid == 1 && got.cls.n_events == 0 && got.cls.pad[0] == 0 && got.cls.pad[1] == 0);
    CHECK(got.on_group < n_groups && (got.off_group <= n_groups));
    // the lowest column of either class: where a class of +inf columns ends up
    std::vector<float> inf(row.size(), INFINITY);
    const Want wi = brute(md, t, n_groups, open, inf);
    CHECK(first_on == wi.col[0] && first_off == wi.col[1]);
    ++n_cases;
}

std::vector<uint32_t> bitmap(int32_t n_groups, const std::vector<int32_t> &open_groups) {
    std::vector<uint32_t> w(static_cast<size_t>(sfa::open_words(n_groups)), 0u);
    for (const int32_t g : open_groups) w[static_cast<size_t>(g / 32)] |= 1u << (g % 32);
    return w;
}

void selftest() {
    const std::vector<int32_t> lens = {1, 31, 32, 33, 64, 65, 300};
    for (int strands = 1; strands <= 2; ++strands)  // 1: RNA, the forward arrays only; 2: DNA
        for (int shift = 0; shift < 2; ++shift) {
            std::vector<int32_t> offs(lens.size(), 0);
            if (shift) offs = {0, 7, 0, 100, 3, 0, 1000};  // ref_st_offset != 0
            const Model md(lens, offs, strands);
            const int32_t o6 = offs[6], o4 = offs[4], o3 = offs[3];
            for (int levels : {3, 1000}) {
                const std::vector<float> row = random_row(md.m.total_cols, levels);
                // overlapping groups: the lower id closed and the higher open, and the reverse; both; neither; null
                const std::vector<sfa_group_target_t> over = {{6, o6 + 10, o6 + 60, 1}, {6, o6 + 40, o6 + 90, 0}, {4, o4 + 5, o4 + 30, 1}};
                for (const std::vector<int32_t> &open : {std::vector<int32_t>{1}, {0}, {0, 1}, {}}) check_record(md, over, 2, bitmap(2, open).data(), row);
                check_record(md, over, 2, nullptr, row);
                // an empty group (1 has no interval, 3 covers no column when the offsets are shifted), open and closed
                const std::vector<sfa_group_target_t> empty = {{3, o3 + 1, o3 + 9, 0}, {3, o3 + 5, o3 + 30, 2}, {3, 0, shift ? 100 : 1, 3}};
                for (const std::vector<int32_t> &open : {std::vector<int32_t>{1, 3}, {0, 1}, {2}, {0, 1, 2, 3}}) check_record(md, empty, 4, bitmap(4, open).data(), row);
                // nothing in a group: the ON class is empty whatever the bitmap says
                check_record(md, {}, 3, bitmap(3, {0, 1, 2}).data(), row);
                // everything in one group
                std::vector<sfa_group_target_t> all;
                for (int32_t r = 0; r < md.m.num_ref; ++r) all.push_back({r, offs[r], offs[r] + lens[r] + 1, 0});
                check_record(md, all, 1, nullptr, row);
                check_record(md, all, 1, bitmap(1, {}).data(), row);
                // bitmaps at the word edges: every column of contig 6 its own group, ids rising by 7 modulo n_groups
                for (const int32_t n_groups : {1, 31, 32, 33, 64, 65, 1023}) {
                    std::vector<sfa_group_target_t> each;
                    for (int32_t c = 0; c < 300; ++c) each.push_back({6, o6 + c, o6 + c + 1, (7 * c) % n_groups});
                    std::vector<int32_t> odd, edges, but_last;
                    for (int32_t g = 0; g < n_groups; ++g) {
                        if (g & 1) odd.push_back(g);
                        if (g == 31 || g == 32 || g == 63 || g == 64 || g == n_groups - 1) edges.push_back(g);
                        if (g != n_groups - 1) but_last.push_back(g);
                    }
                    for (const std::vector<int32_t> &open : {odd, edges, but_last, std::vector<int32_t>{}}) {
                        std::vector<uint32_t> w = bitmap(n_groups, open);
                        check_record(md, each, n_groups, w.data(), row);
                        // set bits at or above n_groups are ignored: the background (label n_groups) and everything behind it
                        const sfa_open_class_t a = record_of(md, each, n_groups, w.data(), row);
                        if (n_groups % 32) w.back() |= ~((1u << (n_groups % 32)) - 1u);
                        const sfa_open_class_t b = record_of(md, each, n_groups, w.data(), row);
                        CHECK(memcmp(&a, &b, sizeof a) == 0);
                        check_record(md, each, n_groups, w.data(), row);
                    }
                    check_record(md, each, n_groups, nullptr, row);
                }
            }
            // classes whose every column costs +inf: the lowest column of the class, not `none`
            {
                std::vector<float> row = random_row(md.m.total_cols, 5);
                const std::vector<sfa_group_target_t> t = {{4, o4 + 10, o4 + 20, 0}, {6, o6 + 100, o6 + 120, 1}};
                std::vector<uint16_t> label;
                sfa::group_labels(t.data(), 2, 2, md.m, &label);
                for (int64_t c = 0; c < md.m.total_cols; ++c)
                    if (label[static_cast<size_t>(c)] == 0) row[static_cast<size_t>(c)] = INFINITY;
                const uint32_t only0 = 1u, only1 = 2u;
                check_record(md, t, 2, &only0, row);
                const sfa_open_class_t r = record_of(md, t, 2, &only0, row);
                CHECK(std::isinf(r.cls.on_score) && r.cls.on_rid == 4 && r.on_group == 0 && std::isfinite(r.cls.off_score));
                check_record(md, t, 2, &only1, row);
            }
        }
    // normalised words: below n_groups the caller's, zero above; null: all open
    for (const int32_t n_groups : {1, 31, 32, 33, 64, 65, 1023}) {
        uint32_t norm[sfa::kOpenWords];
        std::vector<uint32_t> ones(static_cast<size_t>(sfa::open_words(n_groups)), 0xffffffffu);
        CHECK(sfa::open_words(n_groups) == (n_groups + 31) / 32);
        for (const uint32_t *src : {static_cast<const uint32_t *>(nullptr), static_cast<const uint32_t *>(ones.data())}) {
            sfa::open_normalise(src, n_groups, norm);
            for (int32_t g = 0; g < 32 * sfa::kOpenWords; ++g) CHECK(sfa::open_bit(norm, g) == (g < n_groups));
        }
        std::vector<uint32_t> zero(ones.size(), 0u);
        sfa::open_normalise(zero.data(), n_groups, norm);
        for (int32_t g = 0; g < 32 * sfa::kOpenWords; ++g) CHECK(!sfa::open_bit(norm, g));
        ++n_cases;
    }
    // the tie rule is class_before: equal costs in both classes, each class reports its own lowest column
    {
        const Model md({8}, {10}, 1);
        const std::vector<float> row = {5.f, 2.f, 9.f, 2.f, 2.f, INFINITY, 2.f, 7.f};
        const std::vector<sfa_group_target_t> t = {{0, 11, 12, 0}, {0, 13, 14, 1}, {0, 14, 15, 2}, {0, 16, 17, 0}};  // labels 3 0 3 1 2 3 0 3
        for (uint32_t open = 0; open < 8; ++open) {
            check_record(md, t, 3, &open, row);
            const sfa_open_class_t r = record_of(md, t, 3, &open, row);
            int32_t want_on = sfa::kNoColumn, want_off = sfa::kNoColumn;
            float c_on = INFINITY, c_off = INFINITY;
            const int lab[8] = {3, 0, 3, 1, 2, 3, 0, 3};
            for (int32_t col = 7; col >= 0; --col) {  // (falling order: class_before's second clause does the work)
                const bool on = lab[col] < 3 && ((open >> lab[col]) & 1u);
                float &c = on ? c_on : c_off;
                int32_t &g = on ? want_on : want_off;
                if (g == sfa::kNoColumn || sfa::class_before(row[col], col, c, g)) c = row[col], g = col;
            }
            CHECK(r.cls.on_pos_end == (want_on == sfa::kNoColumn ? -1 : 10 + want_on) && r.cls.off_pos_end == (want_off == sfa::kNoColumn ? -1 : 10 + want_off));
            CHECK(r.on_group == (want_on == sfa::kNoColumn ? -1 : lab[want_on]) && r.off_group == lab[want_off]);
        }
        const sfa_open_class_t none = sfa::open_class_none();
        CHECK(none.cls.valid == 0 && std::isinf(none.cls.on_score) && std::isinf(none.cls.off_score) && none.cls.on_rid == -1 && none.cls.off_pos_end == -1 && none.on_group == -1 &&
              none.off_group == -1 && none.cls.on_strand == 0);
    }
    // the quota book
    {
        sfa::QuotaBook b(65, 2);
        CHECK(b.n_words() == 3 && b.open()[0] == 0xffffffffu && b.open()[1] == 0xffffffffu && b.open()[2] == 1u);
        CHECK(!b.note_accept(64) && b.is_open(64) && b.accepted(64) == 1);
        CHECK(b.note_accept(64) && !b.is_open(64) && b.accepted(64) == 2 && b.open()[2] == 0u);  // closes at exactly the quota
        CHECK(!b.note_accept(64) && b.accepted(64) == 3 && !b.is_open(64));                       // a closed group: counted, nothing changes
        CHECK(!b.note_accept(65) && !b.note_accept(-1) && !b.note_accept(1 << 20));                // the background, no group: counted nowhere
        b.set_quota(31, 0);                                                                        // unlimited
        for (int k = 0; k < 1000; ++k) CHECK(!b.note_accept(31));
        CHECK(b.is_open(31) && b.accepted(31) == 1000 && b.quota(31) == 0 && b.quota(32) == 2);
        b.set_quota(32, 1);
        CHECK(b.note_accept(32) && b.open()[1] == 0xfffffffeu && b.open()[0] == 0xffffffffu);
        sfa::QuotaBook all(1023, 1);
        for (int32_t g = 0; g < 1023; ++g) CHECK(all.is_open(g) && all.note_accept(g) && !all.is_open(g));
        for (int w = 0; w < all.n_words(); ++w) CHECK(all.open()[w] == 0u);
        CHECK(!all.is_open(1023) && !all.is_open(-1));
        sfa::QuotaBook free(3, 0);
        for (int k = 0; k < 10; ++k) CHECK(!free.note_accept(k % 3));
        CHECK(free.open()[0] == 7u);
        n_cases += 4;
    }
    printf("selftest ok %d\n", n_cases);
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest")) {
            selftest();
        } else if (!strcmp(word, "record")) {
            int strands, num_ref, n, n_groups, n_words;
            if (scanf("%d %d", &strands, &num_ref) != 2 || num_ref < 1 || num_ref > 4096) return 2;
            std::vector<int32_t> lens(num_ref), offs(num_ref);
            for (int r = 0; r < num_ref; ++r)
                if (scanf("%d %d", &lens[r], &offs[r]) != 2) return 2;
            if (scanf("%d %d", &n_groups, &n) != 2 || n < 0 || n > 1 << 20) return 2;
            std::vector<sfa_group_target_t> t(n);
            for (int k = 0; k < n; ++k)
                if (scanf("%d %d %d %d", &t[k].contig, &t[k].begin, &t[k].end, &t[k].group) != 4) return 2;
            if (scanf("%d", &n_words) != 1 || n_words > sfa::kOpenWords) return 2;
            std::vector<uint32_t> open(n_words > 0 ? n_words : 0);
            for (uint32_t &w : open)
                if (scanf("%x", &w) != 1) return 2;
            const Model md(lens, offs, strands);
            if (n_words >= 0 && n_words != sfa::open_words(n_groups)) return 2;
            std::vector<float> row(static_cast<size_t>(md.m.total_cols));
            for (float &c : row) {
                uint32_t u;
                if (scanf("%x", &u) != 1) return 2;
                memcpy(&c, &u, 4);
            }
            int32_t first_on, first_off;
            const sfa_open_class_t r = record_of(md, t, n_groups, n_words < 0 ? nullptr : open.data(), row, &first_on, &first_off);
            uint32_t a, b;
            memcpy(&a, &r.cls.on_score, 4);
            memcpy(&b, &r.cls.off_score, 4);
            printf("record %08x %08x %d %d %d %d %d %d %d %d %d %d\n", a, b, r.cls.on_rid, r.cls.on_pos_end, r.cls.off_rid, r.cls.off_pos_end, r.cls.on_strand, r.cls.off_strand, r.on_group,
                   r.off_group, first_on, first_off);
        } else if (!strcmp(word, "book")) {
            int n_groups, n;
            long long quota;
            if (scanf("%d %lld %d", &n_groups, &quota, &n) != 3 || n_groups < 1 || n_groups > sfa::kGroupMax || n < 0) return 2;
            sfa::QuotaBook book(n_groups, quota);
            printf("book");
            for (int k = 0; k < n; ++k) {
                int g;
                if (scanf("%d", &g) != 1) return 2;
                printf(" %d", book.note_accept(g) ? 1 : 0);
            }
            printf(" |");
            for (int g = 0; g < n_groups; ++g) printf(" %lld", static_cast<long long>(book.accepted(g)));
            printf(" |");
            for (int w = 0; w < book.n_words(); ++w) printf(" %08x", book.open()[w]);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
