// truth_rules.hpp -- the host rules that check a target decision against where a read really came from (`realtime --truth`,
// replay(truth=); pure C++, no HIP, no context; tests/c/truth_rules.cpp runs them without a GPU).  The targets, the groups, the
// decision and the tie rule of a column are target_rules.hpp's, group_rules.hpp's and quota_rules.hpp's; nothing of them is restated
// here: truth is about a read's own interval, never about a column of a row.
//   * the truth table (TruthTable): one record per read id, (contig, begin, end) or `belongs nowhere`, from a PAF file -- column 1
//     the read id, column 6 the contig's name, columns 8 and 9 begin and end (0-based, half open, forward strand); a contig `*`
//     says the read belongs nowhere and its coordinates are not read.  Empty lines are skipped.  Refused, with file name and line
//     number: fewer than 9 tab-separated columns, a coordinate that is no integer in 0 .. 2^31 - 1, end <= begin, a contig the
//     reference does not have, a read id that appears twice.  A read that is not in the file has no truth.
//   * the true class (truth_class): 'T' when [begin, end) shares at least one base with an interval of its contig, 'O' when it
//     shares none or the read belongs nowhere; a read without truth is 'N' (truth_class_of).  An OVERLAP rule on purpose: the
//     class decision reads the alignment's END coordinate, so a read that straddles an interval's edge can honestly go either
//     way.  truth_edge names such reads: overlapping, but contained in no single interval.
//   * the true group (truth_group): the lowest group id among the overlapping intervals (group_labels' tie rule for a column),
//     else the background, n_groups
//   * the verdict of a decided read (truth_verdict): 'C' when the decided class equals the true one, 'W' when it differs, 'N' when
//     either is 'N'; over groups (truth_group_verdict) the same comparison of two entries, a negative entry being `none`
//   * the account (TruthAccount): per true class reads, samples (sent to the session, held on the channel after the decision, in
//     the file), counts by action and by verdict; integer sums only.  From them the share of the sequenced samples (sent + held:
//     what the pore read) that belong to true-'T' reads, the same share of the file's samples -- what no selection would have
//     sequenced --, and their ratio, the enrichment by signal.  The shares are taken over the reads that HAVE truth ('T' and 'O'):
//     a read without truth may be either.  A quotient is formed only where it is printed and only when its divisor is not 0.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <istream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sigfish_amd.h"

namespace sfa {

struct TruthRecord {
    int32_t contig;  // index into the reference's contigs; -1: the read belongs nowhere
    int32_t begin, end;
};

// ---- the class, the group, the verdicts ----
inline bool truth_shares_a_base(const int32_t begin, const int32_t end, const int32_t t_begin, const int32_t t_end) { return begin < t_end && t_begin < end; }

inline char truth_class(const sfa_target_t *t, const int32_t n, const int32_t contig, const int32_t begin, const int32_t end) {
    if (contig < 0) return 'O';
    for (int32_t k = 0; k < n; ++k)
        if (t[k].contig == contig && truth_shares_a_base(begin, end, t[k].begin, t[k].end)) return 'T';
    return 'O';
}

// overlapping, but contained in no single interval
inline bool truth_edge(const sfa_target_t *t, const int32_t n, const int32_t contig, const int32_t begin, const int32_t end) {
    if (contig < 0) return false;
    bool overlaps = false;
    for (int32_t k = 0; k < n; ++k) {
        if (t[k].contig != contig || !truth_shares_a_base(begin, end, t[k].begin, t[k].end)) continue;
        if (t[k].begin <= begin && end <= t[k].end) return false;
        overlaps = true;
    }
    return overlaps;
}

inline int32_t truth_group(const sfa_group_target_t *t, const int32_t n, const int32_t n_groups, const int32_t contig, const int32_t begin, const int32_t end) {
    int32_t g = n_groups;
    if (contig < 0) return g;
    for (int32_t k = 0; k < n; ++k)
        if (t[k].contig == contig && t[k].group >= 0 && t[k].group < g && truth_shares_a_base(begin, end, t[k].begin, t[k].end)) g = t[k].group;
    return g;
}

// a class is 'T' or 'O'; anything else is 'N', no class
inline char truth_verdict(const int decided, const int truth) {
    const bool d = decided == 'T' || decided == 'O', t = truth == 'T' || truth == 'O';
    return !d || !t ? 'N' : (decided == truth ? 'C' : 'W');
}
inline char truth_group_verdict(const int32_t decided, const int32_t truth) { return decided < 0 || truth < 0 ? 'N' : (decided == truth ? 'C' : 'W'); }

// 'T', 'O', or 'N' for a read without truth (rec null)
inline char truth_class_of(const TruthRecord *rec, const sfa_target_t *t, const int32_t n) { return rec ? truth_class(t, n, rec->contig, rec->begin, rec->end) : 'N'; }

// ---- the truth table ----
class TruthTable {
   public:
    // false: *err holds `path:line: why`
    bool read(std::istream &in, const std::string &path, const std::vector<std::string> &contigs, std::string *err) {
        rec_.clear();
        std::string ln;
        for (long no = 1; std::getline(in, ln); ++no) {
            if (!ln.empty() && ln.back() == '\r') ln.pop_back();
            if (ln.empty()) continue;
            std::string id;
            TruthRecord r;
            const std::string why = parse_line(ln, contigs, &id, &r);
            if (!why.empty() || !rec_.emplace(id, r).second) {
                *err = path + ":" + std::to_string(no) + ": " + (why.empty() ? "read id '" + id + "' appears twice" : why);
                return false;
            }
        }
        return true;
    }
    const TruthRecord *find(const std::string &read_id) const {
        const auto it = rec_.find(read_id);
        return it == rec_.end() ? nullptr : &it->second;
    }
    size_t size() const { return rec_.size(); }

    // one line into (id, record); "" or why it is refused
    static std::string parse_line(const std::string &ln, const std::vector<std::string> &contigs, std::string *id, TruthRecord *r) {
        std::string f[9];
        size_t at = 0;
        for (int k = 0; k < 9; ++k) {
            if (at > ln.size()) return "a PAF line has at least 9 tab-separated columns (this one has " + std::to_string(k) + ")";
            const size_t tab = ln.find('\t', at);
            f[k] = ln.substr(at, tab == std::string::npos ? std::string::npos : tab - at);
            at = tab == std::string::npos ? ln.size() + 1 : tab + 1;
        }
        if (f[0].empty()) return "the read id (column 1) is empty";
        *id = f[0];
        if (f[5] == "*") {
            *r = TruthRecord{-1, 0, 0};
            return "";
        }
        int32_t contig = -1;
        for (size_t c = 0; c < contigs.size(); ++c)
            if (contigs[c] == f[5]) contig = static_cast<int32_t>(c);
        if (contig < 0) return "contig '" + f[5] + "' is not in the reference";
        long long b = 0, e = 0;
        if (!number(f[7], &b) || !number(f[8], &e)) return "begin and end (columns 8 and 9) must be integers in 0 .. 2147483647";
        if (e <= b) return "the interval [" + f[7] + ", " + f[8] + ") is empty";
        *r = TruthRecord{contig, static_cast<int32_t>(b), static_cast<int32_t>(e)};
        return "";
    }

   private:
    static bool number(const std::string &s, long long *v) {
        if (s.empty() || s.size() > 10) return false;
        for (const char c : s)
            if (c < '0' || c > '9') return false;
        *v = strtoll(s.c_str(), nullptr, 10);
        return *v <= INT32_MAX;
    }
    std::unordered_map<std::string, TruthRecord> rec_;
};

// ---- the account ----
struct TruthAccount {
    struct Class {
        int64_t reads = 0, sent = 0, held = 0, file = 0, edge = 0;
        int64_t action[3] = {0, 0, 0};   // A, U, P
        int64_t verdict[3] = {0, 0, 0};  // C, W, N
    };
    Class cls[3];                          // true class T, O, N
    int64_t group_verdict[3] = {0, 0, 0};  // C, W, N of the reads that printed a group

    static int class_index(const char c) { return c == 'T' ? 0 : c == 'O' ? 1 : 2; }
    static int action_index(const char a) { return a == 'A' ? 0 : a == 'U' ? 1 : 2; }
    static int verdict_index(const char v) { return v == 'C' ? 0 : v == 'W' ? 1 : 2; }

    // one decided read: its true class, whether it is an edge read, what happened to it, the verdict, the samples sent to the
    // session up to the decision, those its channel was held for behind it, and the read's length in the file
    void note(const char tt, const bool edge, const char action, const char tv, const int64_t sent, const int64_t held, const int64_t in_file) {
        Class &c = cls[class_index(tt)];
        ++c.reads;
        c.sent += sent, c.held += held, c.file += in_file;
        c.edge += edge ? 1 : 0;
        ++c.action[action_index(action)];
        ++c.verdict[verdict_index(tv)];
    }
    void note_group(const char gv) { ++group_verdict[verdict_index(gv)]; }

    int64_t sequenced(const int k) const { return cls[k].sent + cls[k].held; }
    // numerators and divisors of the two shares (reads with truth only)
    int64_t seq_on() const { return sequenced(0); }
    int64_t seq_all() const { return sequenced(0) + sequenced(1); }
    int64_t file_on() const { return cls[0].file; }
    int64_t file_all() const { return cls[0].file + cls[1].file; }
    bool enrichment_defined() const { return seq_all() > 0 && file_on() > 0; }

    // the `truth:` lines of the summary (Python twin: realtime.format_truth_summary)
    std::string format(const bool groups) const {
        std::string out;
        char buf[512];
        for (int k = 0; k < 3; ++k) {
            const Class &c = cls[k];
            snprintf(buf, sizeof buf, "[realtime] truth: %c reads=%lld sent=%lld held=%lld file=%lld A=%lld U=%lld P=%lld C=%lld W=%lld N=%lld edge=%lld\n", "TON"[k],
                     (long long)c.reads, (long long)c.sent, (long long)c.held, (long long)c.file, (long long)c.action[0], (long long)c.action[1], (long long)c.action[2],
                     (long long)c.verdict[0], (long long)c.verdict[1], (long long)c.verdict[2], (long long)c.edge);
            out += buf;
        }
        if (groups) {
            snprintf(buf, sizeof buf, "[realtime] truth: groups C=%lld W=%lld N=%lld\n", (long long)group_verdict[0], (long long)group_verdict[1], (long long)group_verdict[2]);
            out += buf;
        }
        auto quotient = [](const int64_t a, const int64_t b) -> std::string {  // "-": not formed
            if (b <= 0) return "-";
            char q[32];
            snprintf(q, sizeof q, "%.4f", static_cast<double>(a) / static_cast<double>(b));
            return q;
        };
        std::string ratio = "-";
        if (enrichment_defined()) {
            char q[32];
            snprintf(q, sizeof q, "%.4f", (static_cast<double>(seq_on()) * static_cast<double>(file_all())) / (static_cast<double>(seq_all()) * static_cast<double>(file_on())));
            ratio = q;
        }
        snprintf(buf, sizeof buf, "[realtime] truth: on-target share of the sequenced samples (sent + held) %lld / %lld = %s, of the file's samples %lld / %lld = %s, enrichment by signal %s\n",
                 (long long)seq_on(), (long long)seq_all(), quotient(seq_on(), seq_all()).c_str(), (long long)file_on(), (long long)file_all(), quotient(file_on(), file_all()).c_str(),
                 ratio.c_str());
        out += buf;
        return out;
    }
};

}  // namespace sfa
