// replay.hpp -- the schedule of `sigfish-amd realtime`: which read is on which channel, which samples go out at which tick,
// what happens on a decision.  No device call and no file here: the run (realtime_main.cpp) and tests/c/replay_schedule.cpp
// drive it, the latter with a stub in place of the session.  Python twin: sigfish_amd/realtime.py (Schedule, decide); both
// print the same trace, line for line.
//
// The schedule is defined on ticks, never on wall-clock time:
//   setup     read i of the file goes to channel i, i < channels
//   tick t    every busy channel sends the next chunk_samples samples of its read, channels in ascending order, in ONE call.
//             A chunk shorter than chunk_samples (empty when the read's length is a multiple of it) is the read's last and
//             carries end_of_read
//   decision  after the call every named channel is tested (decide()): early, full, end of read
//   after it  decided channels are reset in one call and each takes the next unread record of the file, lowest channel
//             first, from tick t + 1 on; what is left of a decided read is never sent
//   targets   only with --targets (Schedule's `targets`, end_tick's `action`): a read that is accepted ('A') or proceeds ('P': full
//             or ended without a class decision) keeps its channel for ceil((len - sent) / chunk_samples) further ticks without
//             sending anything -- the pore goes on reading it -- one trace line `hold ... left=K` per such tick, K counting down to
//             1; the channel takes its next read at the end of the last one.  An unblocked read ('U') frees its channel at once.
//             Channels freed in a tick, by a decision or by a hold that ends, take the next records lowest channel first
//   quota     only with --quota (set_quota, end_tick's `on_group`): every read accepted ('A') with a line in the tick is credited to
//             the open group of its best on-target column, ascending channels, in the quota book (quota_rules.hpp; host arithmetic).
//             The credit that fills a group's quota closes it -- trace line `close group=NAME accepted=K` behind the read's
//             `decide` line -- for the ticks that follow: the run asks for a tick's classes under the bitmap as it stood when the
//             tick began, so a tick does not depend on the order of its decisions and a group may overshoot by the reads accepted in
//             its closing tick.  Proceeding reads ('P') are not credited
//   truth     only with --truth (end_tick's `truth`; truth_rules.hpp holds the rules, nothing of them is restated here): behind every
//             `decide` line one line `verdict ch=C read=R tt=X tv=Y sent=S` -- the read's true class, the verdict of its decided
//             class and the samples sent, the decide line's own.  Truth changes no decision: the trace without its verdict lines is
//             the trace of the run without --truth
//   the end   no channel is busy
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../quota_rules.hpp"

namespace cli {
namespace replay {

// what the decision rule reads of a channel's row and raw info after a call
struct Status {
    bool calibrated = false, full = false, ended = false, poisoned = false;
    bool mapped = false;  // the row is valid and names a contig
    int64_t q_events = 0;
    int mapq = 0;
};

struct Rule {
    int64_t min_events;
    int min_mapq;
};

// 'E' early, 'F' full, 'R' end of read (a poisoned slot as well: it can never have a row), 0: the read goes on.
// A decision prints a line when the row is mapped; 'E' always is.
inline char decide(const Rule &r, const Status &s) {
    if (s.calibrated && s.q_events >= r.min_events && s.mapped && s.mapq >= r.min_mapq) return 'E';
    if (s.full) return 'F';
    if (s.ended || s.poisoned) return 'R';
    return 0;
}

// ---- with targets (target_rules.hpp decides; nothing of it is restated here) ----
// The 'E' test of decide() replaced: `decision` is target_decide() of the slot's class result ('A', 'U' or 0).  'F' and 'R' as above.
inline char decide_targets(const Status &s, char decision) {
    if (s.calibrated && decision) return 'E';
    if (s.full) return 'F';
    if (s.ended || s.poisoned) return 'R';
    return 0;
}
// what happens to a decided read: the class decision when it was early, else it proceeds
inline char action_of(char reason, char decision) { return reason == 'E' ? decision : 'P'; }

// ---- with --by-name: the two tags a line gains behind tm:f: (Python twin: realtime.group_tags) ----
// The fields are sfa_group_head_t's: tg:Z: names the best entry (`*`: the background, index names.size(), or no entry), gm:f: is
// (second_score - best_score) / n_events to four decimals with a missing runner-up counting as +inf; nan where undefined (no
// events, no best entry, +inf against +inf).
inline std::string group_tags(int32_t best, int32_t second, float best_score, float second_score, int32_t n_events, const std::vector<std::string> &names) {
    const std::string name = best >= 0 && static_cast<size_t>(best) < names.size() ? names[static_cast<size_t>(best)] : "*";
    const double runner = second < 0 ? static_cast<double>(INFINITY) : static_cast<double>(second_score);
    const double gm = n_events > 0 && best >= 0 ? (runner - static_cast<double>(best_score)) / static_cast<double>(n_events) : static_cast<double>(NAN);
    char buf[64];
    if (std::isnan(gm))
        snprintf(buf, sizeof buf, "\tgm:f:nan");
    else
        snprintf(buf, sizeof buf, "\tgm:f:%.4f", gm);
    return "\ttg:Z:" + name + buf;
}

// ---- with --group-cap: when a group counts as full, and its line of the summary (Python twins: realtime.group_is_full,
// realtime.group_cover_line).  A group without columns is never full and has no mean: the quotient is not formed ----
inline bool group_is_full(int64_t columns, int64_t capped) { return columns > 0 && capped == columns; }
inline std::string group_cover_line(const std::string &name, int64_t columns, int64_t capped, uint64_t depth_sum) {
    char buf[160];
    if (columns > 0)
        snprintf(buf, sizeof buf, "\tcolumns=%ld capped=%ld mean_depth=%.3f\n", (long)columns, (long)capped, static_cast<double>(depth_sum) / static_cast<double>(columns));
    else
        snprintf(buf, sizeof buf, "\tcolumns=0 capped=0 mean_depth=-\n");
    return "[realtime] group depth " + name + buf;
}

// ---- with --quota: the tag a line gains behind gm:f: (Python twin: realtime.quota_tags) ----
// og:Z: names sfa_open_class_t's on_group, the open group the read's best on-target column belongs to; `*`: the ON class is empty
inline std::string quota_tags(int32_t on_group, const std::vector<std::string> &names) {
    return "\tog:Z:" + (on_group >= 0 && static_cast<size_t>(on_group) < names.size() ? names[static_cast<size_t>(on_group)] : std::string("*"));
}

// ---- with --group-lead: the line the summary gains (Python twin: realtime.format_reach_group_summary).  The labelled columns
// are the mask's on-target columns: a label is a group exactly where the reach mask of the same list has its bit ----
inline std::string reach_group_line(int32_t lead, bool stranded, int64_t columns) {
    char buf[128];
    snprintf(buf, sizeof buf, "[realtime] reach groups: lead %d%s\tlabelled columns: %ld\n", lead, stranded ? ", stranded" : "", (long)columns);
    return buf;
}

// ---- with --truth: the two tags a line gains behind all others, and with --by-name two more (Python twin: realtime.truth_tags) ----
// tt:A: the read's true class (T, O; N: the read has no truth), tv:A: the verdict of the line's tc (C, W; N: either is N);
// tn:Z: the true group's name (`*`: the background, `.`: the read has no truth), gv:A: the verdict of the line's tg
inline std::string truth_tags(char tt, char tv) { return std::string("\ttt:A:") + tt + "\ttv:A:" + tv; }
inline std::string truth_group_tags(int32_t true_group, char gv, const std::vector<std::string> &names) {
    const std::string name = true_group < 0 ? "." : (static_cast<size_t>(true_group) < names.size() ? names[static_cast<size_t>(true_group)] : "*");
    return "\ttn:Z:" + name + "\tgv:A:" + gv;
}
// what the schedule prints of a tick's decided reads under --truth: per entry of begin_tick() (undecided entries are not read)
struct TruthMarks {
    std::vector<char> tt, tv;
};

// one channel's part of a tick's call
struct Entry {
    int32_t channel;
    int64_t read;          // position of the read in the file
    int64_t first, count;  // samples [first, first + count) of it
    bool end;              // end_of_read
};

// Source: bool take(int32_t channel, int64_t *n_samples) -- the next unread record of the file goes to `channel`
// (false: the file has no more).  The schedule numbers the records in the order it takes them.
class Schedule {
  public:
    Schedule(int32_t channels, int64_t chunk_samples, FILE *trace = nullptr, bool targets = false) : chunk_(chunk_samples), trace_(trace), targets_(targets), ch_(channels) {}

    template <class Source>
    void start(Source &src) {
        for (int32_t c = 0; c < static_cast<int32_t>(ch_.size()); ++c)
            if (!take(c, src)) break;
    }
    // --quota: the book the accepted reads are credited in and the groups' names (both outlive the schedule)
    void set_quota(sfa::QuotaBook *book, const std::vector<std::string> *names) {
        book_ = book, names_ = names;
        closed_at_.assign(static_cast<size_t>(book->n_groups()), -1);
    }
    int64_t closed_at(int32_t group) const { return closed_at_[static_cast<size_t>(group)]; }  // the tick whose credit closed the group, -1: open
    bool busy() const { return n_busy_ > 0; }
    int64_t tick() const { return tick_; }
    int64_t reads_taken() const { return next_read_; }
    int64_t sent(int32_t channel) const { return ch_[channel].sent; }
    int64_t length(int32_t channel) const { return ch_[channel].len; }

    // the entries of the next call, ascending channels; their samples count as sent
    const std::vector<Entry> &begin_tick() {
        entries_.clear();
        for (int32_t c = 0; c < static_cast<int32_t>(ch_.size()); ++c) {
            Channel &k = ch_[c];
            if (k.read < 0) continue;
            if (k.hold > 0) {  // (only with targets)
                if (trace_) fprintf(trace_, "tick %ld hold ch=%d read=%ld left=%ld\n", (long)tick_, c, (long)k.read, (long)k.hold);
                continue;
            }
            const int64_t left = k.len - k.sent, n = left < chunk_ ? left : chunk_;
            entries_.push_back(Entry{c, k.read, k.sent, n, n < chunk_});
            k.sent += n;
            if (trace_)
                fprintf(trace_, "tick %ld send ch=%d read=%ld first=%ld n=%ld end=%d\n", (long)tick_, c, (long)k.read, (long)entries_.back().first, (long)n, n < chunk_ ? 1 : 0);
        }
        return entries_;
    }

    // reason[i] (decide()) and line[i] for entry i of begin_tick(); decided channels take the next records, lowest channel first.
    // With targets, action[i] (action_of) says what happens to a decided read; *held (if given) receives the samples a read
    // decided in this tick is held for.  With truth, a `verdict` line follows every `decide` line.
    template <class Source>
    void end_tick(const std::vector<char> &reason, const std::vector<char> &line, Source &src, const std::vector<char> *action = nullptr, std::vector<int64_t> *held = nullptr,
                  const std::vector<int32_t> *on_group = nullptr, const TruthMarks *truth = nullptr) {
        if (!targets_ || !action) {
            for (size_t i = 0; i < entries_.size(); ++i) {
                if (!reason[i]) continue;
                const Entry &e = entries_[i];
                if (trace_)
                    fprintf(trace_, "tick %ld decide ch=%d read=%ld reason=%c line=%d sent=%ld\n", (long)tick_, e.channel, (long)e.read, reason[i], line[i] ? 1 : 0, (long)ch_[e.channel].sent);
                ch_[e.channel].read = -1;
                --n_busy_;
            }
            for (size_t i = 0; i < entries_.size(); ++i)
                if (reason[i] && !take(entries_[i].channel, src)) break;
            ++tick_;
            return;
        }
        if (held) held->assign(entries_.size(), 0);
        std::vector<char> freed(ch_.size(), 0);
        for (int32_t c = 0; c < static_cast<int32_t>(ch_.size()); ++c)  // holds of earlier ticks: one tick less, the last one frees
            if (ch_[c].read >= 0 && ch_[c].hold > 0 && --ch_[c].hold == 0) freed[c] = 1;
        for (size_t i = 0; i < entries_.size(); ++i) {
            if (!reason[i]) continue;
            const Entry &e = entries_[i];
            Channel &k = ch_[e.channel];
            if (trace_)
                fprintf(trace_, "tick %ld decide ch=%d read=%ld reason=%c line=%d sent=%ld\n", (long)tick_, e.channel, (long)e.read, reason[i], line[i] ? 1 : 0, (long)k.sent);
            if (trace_ && truth) fprintf(trace_, "tick %ld verdict ch=%d read=%ld tt=%c tv=%c sent=%ld\n", (long)tick_, e.channel, (long)e.read, truth->tt[i], truth->tv[i], (long)k.sent);
            if (book_ && on_group && (*action)[i] == 'A' && line[i] && book_->note_accept((*on_group)[i])) {  // this read filled its group's quota
                const int32_t g = (*on_group)[i];
                closed_at_[static_cast<size_t>(g)] = tick_;
                if (trace_) fprintf(trace_, "tick %ld close group=%s accepted=%ld\n", (long)tick_, (*names_)[static_cast<size_t>(g)].c_str(), (long)book_->accepted(g));
            }
            const int64_t ticks = (*action)[i] == 'U' ? 0 : (k.len - k.sent + chunk_ - 1) / chunk_;
            if (ticks > 0) {
                k.hold = ticks;
                if (held) (*held)[i] = k.len - k.sent;
            } else {
                freed[e.channel] = 1;
            }
        }
        bool more = true;
        for (int32_t c = 0; c < static_cast<int32_t>(ch_.size()); ++c) {
            if (!freed[c]) continue;
            ch_[c] = Channel{};
            --n_busy_;
            if (more) more = take(c, src);
        }
        ++tick_;
    }

  private:
    struct Channel {
        int64_t read = -1, len = 0, sent = 0;
        int64_t hold = 0;  // ticks the channel still keeps a decided read without sending (targets)
    };
    template <class Source>
    bool take(int32_t c, Source &src) {
        int64_t len = 0;
        if (!src.take(c, &len)) return false;
        ch_[c] = Channel{next_read_++, len, 0, 0};
        ++n_busy_;
        if (trace_) fprintf(trace_, "tick %ld take ch=%d read=%ld len=%ld\n", (long)tick_, c, (long)ch_[c].read, (long)len);
        return true;
    }
    const int64_t chunk_;
    FILE *trace_;
    const bool targets_;
    sfa::QuotaBook *book_ = nullptr;  // --quota
    const std::vector<std::string> *names_ = nullptr;
    std::vector<int64_t> closed_at_;
    std::vector<Channel> ch_;
    std::vector<Entry> entries_;
    int64_t tick_ = 0, next_read_ = 0;
    int32_t n_busy_ = 0;
};

}  // namespace replay
}  // namespace cli
