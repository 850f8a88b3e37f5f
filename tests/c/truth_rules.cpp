// The host rules of `realtime --truth` (sigfish_amd/csrc/truth_rules.hpp) as a stand-alone host program, built from that header
// alone; tests/test_truth_rules_cpu.py runs it plain and under ASan + UBSan.
//   selftest      overlap by exactly one base at either end of a target, a target that touches but does not overlap, containment
//                 against `edge`, a read over targets of two groups, a read that belongs nowhere, an absent read, every refusal of
//                 the parser with its line number, the verdicts, the account's sums on a hand-made list, an all-N account (no
//                 quotient is formed); the class and the group against a base-by-base brute force on random intervals.  Prints
//                 "selftest ok <cases>".
//   parse <n> <contig name per contig> <path>
//                 "ok <records>" and one line "<read id> <contig> <begin> <end>" per id asked for behind it on the same line
//                 (`-`: the id has no truth), or "error <text>"
//   account <groups 0|1> <n> <tt edge action tv sent held file per read> <m> <gv per group verdict>
//                 the `truth:` lines of the account
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "truth_rules.hpp"

namespace {

int n_cases = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                 \
        }                                                            \
        ++n_cases;                                                   \
    } while (0)

uint32_t rng_state = 2468;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// "" or the refusal of a file with these lines
std::string refusal(const std::string &text, const std::vector<std::string> &names, sfa::TruthTable *table = nullptr) {
    std::istringstream in(text);
    sfa::TruthTable local;
    std::string err;
    return (table ? table : &local)->read(in, "t.paf", names, &err) ? "" : err;
}

std::string paf(const std::string &id, const std::string &contig, const std::string &b, const std::string &e) {
    return id + "\t1000\t0\t1000\t+\t" + contig + "\t5000\t" + b + "\t" + e + "\t10\t10\t60\n";
}

bool starts(const std::string &s, const std::string &p) { return s.compare(0, p.size(), p) == 0; }

void selftest() {
    // targets [100, 200) and [300, 400) of contig 0, [0, 50) of contig 1
    const std::vector<sfa_target_t> t = {{0, 100, 200}, {0, 300, 400}, {1, 0, 50}};
    const int32_t n = static_cast<int32_t>(t.size());
    auto cls = [&](int32_t c, int32_t b, int32_t e) { return sfa::truth_class(t.data(), n, c, b, e); };
    auto edge = [&](int32_t c, int32_t b, int32_t e) { return sfa::truth_edge(t.data(), n, c, b, e); };
    // overlap by exactly one base at either end
    CHECK(cls(0, 50, 101) == 'T' && edge(0, 50, 101));
    CHECK(cls(0, 199, 250) == 'T' && edge(0, 199, 250));
    // touching without overlap: end == begin of the target, begin == end of the target
    CHECK(cls(0, 50, 100) == 'O' && !edge(0, 50, 100));
    CHECK(cls(0, 200, 300) == 'O' && !edge(0, 200, 300));
    // containment against edge
    CHECK(cls(0, 100, 200) == 'T' && !edge(0, 100, 200));
    CHECK(cls(0, 120, 121) == 'T' && !edge(0, 120, 121));
    CHECK(cls(0, 99, 200) == 'T' && edge(0, 99, 200) && cls(0, 100, 201) == 'T' && edge(0, 100, 201));
    CHECK(cls(0, 150, 350) == 'T' && edge(0, 150, 350));  // over two targets, inside neither
    CHECK(cls(0, 0, 5000) == 'T' && edge(0, 0, 5000));
    // the contig matters
    CHECK(cls(1, 100, 200) == 'O' && cls(1, 49, 60) == 'T' && cls(2, 0, 50) == 'O');
    // a read that belongs nowhere; no targets at all
    CHECK(cls(-1, 0, 0) == 'O' && !edge(-1, 100, 200) && cls(-1, 100, 200) == 'O');
    CHECK(sfa::truth_class(nullptr, 0, 0, 100, 200) == 'O' && !sfa::truth_edge(nullptr, 0, 0, 100, 200));
    // a nested target makes a read inside it no edge read, whatever the outer one's edge does
    {
        const std::vector<sfa_target_t> nest = {{0, 100, 200}, {0, 150, 400}};
        CHECK(!sfa::truth_edge(nest.data(), 2, 0, 160, 390) && sfa::truth_edge(nest.data(), 2, 0, 120, 390));
    }
    // groups: the lowest id among the overlapping intervals, else the background
    const std::vector<sfa_group_target_t> g = {{0, 100, 200, 2}, {0, 150, 400, 1}, {0, 390, 500, 0}, {1, 0, 50, 3}};
    auto grp = [&](int32_t c, int32_t b, int32_t e) { return sfa::truth_group(g.data(), static_cast<int32_t>(g.size()), 4, c, b, e); };
    CHECK(grp(0, 100, 150) == 2 && grp(0, 100, 151) == 1 && grp(0, 149, 391) == 0 && grp(0, 400, 401) == 0 && grp(0, 0, 100) == 4);
    CHECK(grp(1, 10, 20) == 3 && grp(1, 50, 60) == 4 && grp(-1, 100, 200) == 4 && grp(2, 100, 200) == 4);
    CHECK(sfa::truth_group(nullptr, 0, 7, 0, 1, 2) == 7);
    // verdicts
    CHECK(sfa::truth_verdict('T', 'T') == 'C' && sfa::truth_verdict('O', 'O') == 'C' && sfa::truth_verdict('T', 'O') == 'W' && sfa::truth_verdict('O', 'T') == 'W');
    CHECK(sfa::truth_verdict('N', 'T') == 'N' && sfa::truth_verdict('T', 'N') == 'N' && sfa::truth_verdict('N', 'N') == 'N' && sfa::truth_verdict(0, 'O') == 'N' &&
          sfa::truth_verdict('C', 'C') == 'N');
    CHECK(sfa::truth_group_verdict(2, 2) == 'C' && sfa::truth_group_verdict(2, 4) == 'W' && sfa::truth_group_verdict(-1, 2) == 'N' && sfa::truth_group_verdict(2, -1) == 'N' &&
          sfa::truth_group_verdict(0, 0) == 'C');

    // ---- the class and the group against a base-by-base brute force ----
    for (int round = 0; round < 400; ++round) {
        std::vector<sfa_target_t> rt;
        std::vector<sfa_group_target_t> rg;
        const int32_t n_groups = 1 + static_cast<int32_t>(rnd() % 5);
        const int nt = static_cast<int>(rnd() % 6);
        for (int k = 0; k < nt; ++k) {
            const int32_t c = static_cast<int32_t>(rnd() % 2), b = static_cast<int32_t>(rnd() % 60), e = b + 1 + static_cast<int32_t>(rnd() % 20);
            rt.push_back({c, b, e});
            rg.push_back({c, b, e, static_cast<int32_t>(rnd() % n_groups)});
        }
        for (int q = 0; q < 8; ++q) {
            const int32_t c = static_cast<int32_t>(rnd() % 3) - 1, b = static_cast<int32_t>(rnd() % 70), e = b + 1 + static_cast<int32_t>(rnd() % 25);
            bool on = false, inside_one = false;
            int32_t group = n_groups;
            for (size_t k = 0; k < rt.size(); ++k) {
                if (rt[k].contig != c) continue;
                int shared = 0;
                for (int32_t x = b; x < e; ++x) shared += rt[k].begin <= x && x < rt[k].end;
                if (shared) on = true, group = std::min(group, rg[k].group);
                if (shared == e - b) inside_one = true;
            }
            CHECK(sfa::truth_class(rt.data(), nt, c, b, e) == (on ? 'T' : 'O'));
            CHECK(sfa::truth_edge(rt.data(), nt, c, b, e) == (on && !inside_one));
            CHECK(sfa::truth_group(rg.data(), nt, n_groups, c, b, e) == group);
        }
    }

    // ---- the parser ----
    const std::vector<std::string> names = {"chrA", "chrB"};
    {
        sfa::TruthTable table;
        const std::string text = paf("r0", "chrA", "100", "200") + "\n" + paf("r1", "*", "0", "0") + paf("r2", "chrB", "0", "2147483647") + "r3\t1\t0\t1\t-\tchrB\t9\t7\t9\r\n" +
                                 paf("r4", "*", "x", "");
        CHECK(refusal(text, names, &table) == "" && table.size() == 5);
        const sfa::TruthRecord *r0 = table.find("r0"), *r1 = table.find("r1"), *r2 = table.find("r2"), *r3 = table.find("r3");
        CHECK(r0 && r0->contig == 0 && r0->begin == 100 && r0->end == 200);
        CHECK(r1 && r1->contig == -1);                                  // belongs nowhere
        CHECK(r2 && r2->contig == 1 && r2->end == 2147483647);
        CHECK(r3 && r3->contig == 1 && r3->begin == 7 && r3->end == 9);  // nine columns are enough; \r\n line ends
        CHECK(table.find("r4") && table.find("r4")->contig == -1);      // the coordinates of a `*` read are not read
        CHECK(table.find("r5") == nullptr && table.find("") == nullptr);  // an absent read has no truth
        CHECK(sfa::truth_class_of(r0, t.data(), n) == 'T' && sfa::truth_class_of(r1, t.data(), n) == 'O' && sfa::truth_class_of(nullptr, t.data(), n) == 'N');
        CHECK(sfa::truth_class_of(r2, t.data(), n) == 'T' && sfa::truth_class_of(r3, t.data(), n) == 'T');
    }
    const std::string good = paf("a", "chrA", "1", "2");
    CHECK(starts(refusal(good + "b\t1\t0\t1\t+\tchrA\t9\t7\n", names), "t.paf:2: a PAF line has at least 9 tab-separated columns (this one has 8)"));
    CHECK(starts(refusal("b c d e f g h i j\n", names), "t.paf:1: a PAF line has at least 9"));  // blanks are no tabs
    CHECK(starts(refusal(good + "\n\n" + paf("b", "chrA", "x", "9"), names), "t.paf:4: begin and end"));
    CHECK(starts(refusal(good + paf("b", "chrA", "1", "9.5"), names), "t.paf:2: begin and end"));
    CHECK(starts(refusal(good + paf("b", "chrA", "-1", "9"), names), "t.paf:2: begin and end"));
    CHECK(starts(refusal(good + paf("b", "chrA", "", "9"), names), "t.paf:2: begin and end"));
    CHECK(starts(refusal(good + paf("b", "chrA", "1", "2147483648"), names), "t.paf:2: begin and end"));
    CHECK(starts(refusal(good + paf("b", "chrA", "1", "99999999999999999999"), names), "t.paf:2: begin and end"));
    CHECK(starts(refusal(good + paf("b", "chrA", "9", "9"), names), "t.paf:2: the interval [9, 9) is empty"));
    CHECK(starts(refusal(paf("b", "chrA", "9", "8"), names), "t.paf:1: the interval [9, 8) is empty"));
    CHECK(starts(refusal(good + paf("b", "chrC", "1", "2"), names), "t.paf:2: contig 'chrC' is not in the reference"));
    CHECK(starts(refusal(good + paf("b", "chrB", "1", "2") + paf("a", "chrB", "5", "6"), names), "t.paf:3: read id 'a' appears twice"));
    CHECK(starts(refusal(good + paf("a", "*", "0", "0"), names), "t.paf:2: read id 'a' appears twice"));
    CHECK(starts(refusal(paf("", "chrA", "1", "2"), names), "t.paf:1: the read id"));
    CHECK(refusal("", names) == "" && refusal("\n\r\n", names) == "");

    // ---- the account on a hand-made list ----
    {
        sfa::TruthAccount a;
        a.note('T', false, 'A', 'C', 1000, 4000, 5000);
        a.note('T', true, 'U', 'W', 800, 0, 3000);
        a.note('T', false, 'P', 'N', 2000, 0, 2000);
        a.note('O', false, 'U', 'C', 500, 0, 6000);
        a.note('O', false, 'A', 'W', 700, 3300, 4000);
        a.note('N', false, 'P', 'N', 900, 100, 1000);
        a.note_group('C'), a.note_group('W'), a.note_group('W'), a.note_group('N');
        CHECK(a.cls[0].reads == 3 && a.cls[0].sent == 3800 && a.cls[0].held == 4000 && a.cls[0].file == 10000 && a.cls[0].edge == 1);
        CHECK(a.cls[0].action[0] == 1 && a.cls[0].action[1] == 1 && a.cls[0].action[2] == 1 && a.cls[0].verdict[0] == 1 && a.cls[0].verdict[1] == 1 && a.cls[0].verdict[2] == 1);
        CHECK(a.cls[1].reads == 2 && a.cls[1].sent == 1200 && a.cls[1].held == 3300 && a.cls[1].file == 10000 && a.cls[1].action[0] == 1 && a.cls[1].action[1] == 1);
        CHECK(a.cls[2].reads == 1 && a.cls[2].sent == 900 && a.cls[2].held == 100 && a.cls[2].file == 1000 && a.cls[2].verdict[2] == 1);
        CHECK(a.group_verdict[0] == 1 && a.group_verdict[1] == 2 && a.group_verdict[2] == 1);
        // the shares are over the reads with truth: 7800 of 12300 sequenced, 10000 of 20000 in the file
        CHECK(a.seq_on() == 7800 && a.seq_all() == 12300 && a.file_on() == 10000 && a.file_all() == 20000 && a.enrichment_defined());
        const std::string text = a.format(true);
        CHECK(text.find("truth: T reads=3 sent=3800 held=4000 file=10000 A=1 U=1 P=1 C=1 W=1 N=1 edge=1\n") != std::string::npos);
        CHECK(text.find("truth: groups C=1 W=2 N=1\n") != std::string::npos);
        CHECK(text.find("7800 / 12300 = 0.6341, of the file's samples 10000 / 20000 = 0.5000, enrichment by signal 1.2683\n") != std::string::npos);
        CHECK(a.format(false).find("groups") == std::string::npos);
    }
    // an all-N file: nothing has truth, no quotient is formed (UBSan would name a division by zero)
    {
        sfa::TruthAccount a;
        for (int k = 0; k < 5; ++k) a.note('N', false, k % 2 ? 'A' : 'U', 'N', 100 * k, 10, 1000);
        CHECK(a.seq_all() == 0 && a.file_all() == 0 && !a.enrichment_defined() && a.cls[2].reads == 5);
        CHECK(a.format(false).find("0 / 0 = -, of the file's samples 0 / 0 = -, enrichment by signal -\n") != std::string::npos);
        sfa::TruthAccount none;
        CHECK(none.format(true).find("enrichment by signal -\n") != std::string::npos);
        // only off-target reads: the shares exist (0), the ratio does not
        sfa::TruthAccount off;
        off.note('O', false, 'U', 'C', 500, 0, 900);
        CHECK(!off.enrichment_defined() && off.format(false).find("0 / 500 = 0.0000, of the file's samples 0 / 900 = 0.0000, enrichment by signal -\n") != std::string::npos);
    }
    printf("selftest ok %d\n", n_cases);
}

}  // namespace

int main() {
    char word[32];
    while (scanf("%31s", word) == 1) {
        if (!strcmp(word, "selftest")) {
            selftest();
        } else if (!strcmp(word, "parse")) {
            int n;
            if (scanf("%d", &n) != 1 || n < 0 || n > 4096) return 2;
            std::vector<std::string> names(n);
            char buf[512];
            for (std::string &s : names) {
                if (scanf("%511s", buf) != 1) return 2;
                s = buf;
            }
            if (scanf("%511s", buf) != 1) return 2;
            const std::string path = buf;
            std::string rest;  // the ids asked for, up to the end of the line
            for (int c; (c = getchar()) != EOF && c != '\n';) rest += static_cast<char>(c);
            std::ifstream in(path);
            if (!in) return 2;
            sfa::TruthTable table;
            std::string err;
            if (!table.read(in, path, names, &err)) {
                printf("error %s\n", err.c_str());
                continue;
            }
            printf("ok %zu\n", table.size());
            std::istringstream ids(rest);
            for (std::string id; ids >> id;) {
                const sfa::TruthRecord *r = table.find(id);
                if (r)
                    printf("%s %d %d %d\n", id.c_str(), r->contig, r->begin, r->end);
                else
                    printf("%s -\n", id.c_str());
            }
        } else if (!strcmp(word, "account")) {
            int groups, n, m;
            if (scanf("%d %d", &groups, &n) != 2 || n < 0) return 2;
            sfa::TruthAccount a;
            for (int k = 0; k < n; ++k) {
                char tt, action, tv;
                int edge;
                long long sent, held, file;
                if (scanf(" %c %d %c %c %lld %lld %lld", &tt, &edge, &action, &tv, &sent, &held, &file) != 7) return 2;
                a.note(tt, edge != 0, action, tv, sent, held, file);
            }
            if (scanf("%d", &m) != 1 || m < 0) return 2;
            for (int k = 0; k < m; ++k) {
                char gv;
                if (scanf(" %c", &gv) != 1) return 2;
                a.note_group(gv);
            }
            fputs(a.format(groups != 0).c_str(), stdout);
        } else {
            return 2;
        }
    }
    return 0;
}
