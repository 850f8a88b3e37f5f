// realtime_main.cpp -- `sigfish-amd realtime`: a BLOW5 file replayed through a raw-signal session as a flow cell would deliver
// it (the schedule: replay.hpp), a PAF line at the moment a read is decided, and the time a tick takes against the signal time
// it stands for.  The hot path is the library's (sfa_session_extend_raw: detector, normalisation -- frozen, or growing with the
// read under --recalibrate; with --resweep swept only when that window changes, which is what direct RNA without --invert
// needs --, sweep); what runs here
// is the staging of a tick's samples, the decision rule and the printing.  With --spread the session's channels are dealt over
// every GPU of --device (SFA_SESSION_SPREAD); the schedule counts ticks, so the output is the same bytes.
// With --by-name the BED file's name column also sets the session's target groups: each tick ends with one
// sfa_session_group_bests call over the channels that print a line, and their lines gain tg / gm (replay::group_tags).
// With --quota N the tick's class call is sfa_session_open_classes under the bitmap of the groups that still want reads, as it stood
// when the tick began; the schedule credits the accepted reads and closes groups (replay.hpp), lines gain og (replay::quota_tags).
// With --targets the early decision is the class decision (sfa_session_classes + sfa_target_decide, one call per tick), lines
// gain the tc / ac / tm tags (target_tags) and accepted reads hold their channels (replay.hpp).
// With --depth-cap N (mask targets, --enrich) the session keeps a depth track (sfa_session_coverage_config); at the end of a tick the
// reads accepted in it add the target interval of the PAF line just printed for them, [pos_st, pos_end) of their contig, in ONE
// sfa_session_coverage_add call, channels ascending, and the live mask it derives holds from the next tick on (trace: `cover` lines).
// With --truth FILE.paf every decided read is looked up once in the truth table (truth_rules.hpp: the rules and the account), when it
// is decided: lines gain tt / tv (tn / gv with --by-name), the trace `verdict` lines, the summary `truth:` lines.  The file is read
// and checked against the FASTA's contig names before the BLOW5 file or a device is opened; no decision reads it.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <deque>
#include <fstream>
#include <sstream>
#include <future>
#include <thread>

#include "../truth_rules.hpp"
#include "replay.hpp"
#include "run.hpp"

namespace cli {
namespace {

struct Context {  // destroyed on every way out, after the helper thread that decodes ahead
    sfa_ctx_t *c = nullptr;
    ~Context() { sfa_destroy(c); }
};

// Records of upcoming reads, decoded on the -t host threads ahead of need: at most `window` of them are decoded and waiting (or
// being decoded), so the whole file is never resident.  The reader is touched by one helper at a time; the main thread only
// collects what a helper has finished.
class ReadAhead {
  public:
    ReadAhead(sfa::Blow5Reader &reader, WorkerPool &pool, size_t window) : reader_(reader), pool_(pool), window_(window) {}
    // start decoding more when half the window is free and nothing is on its way
    void top_up() {
        if (pending_.valid() || eof_ || ready_.size() > window_ / 2) return;
        const size_t want = window_ - ready_.size();
        pending_ = std::async(std::launch::async, [this, want] { return fetch(want); });
    }
    // the next record of the file (false: there is none)
    bool pop(sfa::Blow5Record *out) {
        while (ready_.empty()) {
            if (!pending_.valid()) {
                if (eof_) return false;
                top_up();
            }
            Fetched f = pending_.get();
            eof_ = f.eof;
            for (auto &r : f.recs) ready_.push_back(std::move(r));
        }
        *out = std::move(ready_.front());
        ready_.pop_front();
        return true;
    }

  private:
    struct Fetched {
        std::vector<sfa::Blow5Record> recs;
        bool eof = false;
    };
    Fetched fetch(size_t want) {
        Fetched f;
        std::vector<const uint8_t *> view;
        std::vector<size_t> size;
        std::vector<std::vector<uint8_t>> mem;
        while (view.size() < want) {
            const uint8_t *v = nullptr;
            size_t n = 0;
            int rc = reader_.next_view(&v, &n);
            if (rc == -2) {  // not mappable: copy the record
                mem.emplace_back();
                rc = reader_.next_mem(&mem.back());
                n = mem.back().size();
            }
            if (rc < 0) die(reader_.error());
            if (rc == 0) {
                f.eof = true;
                break;
            }
            view.push_back(v);
            size.push_back(n);
        }
        for (size_t i = 0, m = 0; i < view.size(); ++i)
            if (!view[i]) view[i] = mem[m++].data();  // (after the last emplace_back: the vectors no longer move)
        f.recs.resize(view.size());
        std::atomic<int> bad(0);
        pool_.run(static_cast<int64_t>(view.size()), [&](int64_t i) {
            std::string err;
            if (!reader_.parse(view[i], size[i], &f.recs[i], &err)) bad = 1;
        });
        if (bad) die("error parsing a BLOW5 record");
        return f;
    }
    sfa::Blow5Reader &reader_;
    WorkerPool &pool_;
    const size_t window_;
    std::deque<sfa::Blow5Record> ready_;
    bool eof_ = false;
    std::future<Fetched> pending_;  // (last: its thread is joined before the queue goes)
};

// the reads on the channels, and where the schedule gets the next one from
struct Channels {
    ReadAhead &ahead;
    std::vector<sfa::Blow5Record> rec;
    int64_t reads = 0, samples_in_file = 0;
    double sampling_rate = 0;  // of the first read
    bool take(int32_t channel, int64_t *n_samples) {
        if (!ahead.pop(&rec[channel])) return false;
        if (reads++ == 0) sampling_rate = rec[channel].sampling_rate;
        samples_in_file += static_cast<int64_t>(rec[channel].raw.size());
        *n_samples = static_cast<int64_t>(rec[channel].raw.size());
        return true;
    }
};

// --targets: the BED file as the session's targets -- three columns, `#` / track / browser lines skipped, an unknown contig is an error.
// --by-name (groups, names given): column 4 names the interval's group, numbered by first appearance
std::vector<sfa_target_t> read_targets(const std::string &path, const Reference &ref, std::vector<sfa_group_target_t> *groups = nullptr,
                                       std::vector<std::string> *names = nullptr) {
    std::ifstream in(path);
    if (!in) die("realtime: cannot open the targets file " + path);
    std::vector<sfa_target_t> out;
    std::string ln;
    for (int no = 1; std::getline(in, ln); ++no) {
        std::istringstream f(ln);
        std::string name;
        if (!(f >> name) || name[0] == '#' || name == "track" || name == "browser") continue;
        long b = 0, e = 0;
        if (!(f >> b >> e)) die("realtime: " + path + ":" + std::to_string(no) + ": a BED line has three columns: contig, begin, end");
        int32_t rid = -1;
        for (size_t r = 0; r < ref.contigs.size(); ++r)
            if (ref.contigs[r].name == name) rid = static_cast<int32_t>(r);
        if (rid < 0) die("realtime: " + path + ":" + std::to_string(no) + ": contig '" + name + "' is not in the reference");
        if (b < INT32_MIN || b > INT32_MAX || e < INT32_MIN || e > INT32_MAX) die("realtime: " + path + ":" + std::to_string(no) + ": coordinate out of range");
        out.push_back(sfa_target_t{rid, static_cast<int32_t>(b), static_cast<int32_t>(e)});
        if (groups) {
            std::string group;
            if (ln.find('\t') != std::string::npos) {  // (tab-separated: the name is the fourth field, blanks and all)
                std::istringstream g(ln);
                for (int k = 0; k < 4; ++k)
                    if (!std::getline(g, group, '\t')) group.clear();
                const size_t a = group.find_first_not_of(" \r"), z = group.find_last_not_of(" \r");
                group = a == std::string::npos ? "" : group.substr(a, z - a + 1);
            } else if (!(f >> group)) {
                group.clear();
            }
            if (group.empty()) die("realtime: " + path + ":" + std::to_string(no) + ": --by-name needs a fourth column, the group's name");
            size_t id = 0;
            while (id < names->size() && (*names)[id] != group) ++id;
            if (id == names->size()) {
                if (names->size() == 1023) die("realtime: " + path + ":" + std::to_string(no) + ": more than 1023 group names");
                names->push_back(group);
            }
            groups->push_back(sfa_group_target_t{rid, static_cast<int32_t>(b), static_cast<int32_t>(e), static_cast<int32_t>(id)});
        }
    }
    return out;
}

// --stranded: column 6 of every interval line of the BED file, in the order read_targets keeps them: '+', '-', or 0 for '.'
std::vector<int8_t> read_strands(const std::string &path, const char *option = "--stranded") {
    std::ifstream in(path);
    if (!in) die("realtime: cannot open the targets file " + path);
    std::vector<int8_t> out;
    std::string ln;
    for (int no = 1; std::getline(in, ln); ++no) {
        std::istringstream f(ln);
        std::string name;
        if (!(f >> name) || name[0] == '#' || name == "track" || name == "browser") continue;
        std::string field;
        bool have = true;
        if (ln.find('\t') != std::string::npos) {  // (tab-separated, as read_targets takes column 4)
            std::istringstream g(ln);
            for (int k = 0; k < 6 && have; ++k) have = static_cast<bool>(std::getline(g, field, '\t'));
            const size_t a = field.find_first_not_of(" \r"), z = field.find_last_not_of(" \r");
            field = (!have || a == std::string::npos) ? "" : field.substr(a, z - a + 1);
        } else {
            for (int k = 1; k < 6 && have; ++k) have = static_cast<bool>(f >> field);
            if (!have) field.clear();
        }
        if (field.empty()) die("realtime: " + path + ":" + std::to_string(no) + ": " + option + " needs a sixth column, the strand");
        if (field != "+" && field != "-" && field != ".") die("realtime: " + path + ":" + std::to_string(no) + ": strand '" + field + "' is none of '+', '-', '.'");
        out.push_back(field == "." ? 0 : static_cast<int8_t>(field[0]));
    }
    return out;
}

// --truth: the table of the PAF file, contigs by the names of the FASTA file (read here for its names only: the reference proper is
// built after the BLOW5 file has told the chemistry)
sfa::TruthTable read_truth(const std::string &path, const std::string &fasta) {
    std::vector<sfa::FastaRecord> recs;
    std::string err;
    if (!sfa::read_fasta(fasta, &recs, &err)) die(err);
    std::vector<std::string> names;
    for (const sfa::FastaRecord &c : recs) names.push_back(c.name);
    std::ifstream in(path);
    if (!in) die("realtime: cannot open the truth file " + path);
    sfa::TruthTable table;
    if (!table.read(in, path, names, &err)) die("realtime: " + err);
    return table;
}

// the class a decision stands for: 'T' on target, 'O' off target, 'N' none (dec: sfa_target_decide's 'A', 'U' or 0)
char class_of_decision(int dec, int target_mode) { return !dec ? 'N' : (((dec == 'A') == (target_mode == 0)) ? 'T' : 'O'); }

// the three tags a line gains with --targets (Python twin: realtime.target_tags): class, action, the per-event margin it had
std::string target_tags(const sfa_class_t &c, const RealtimeOpt &r) {
    const int dec = sfa_target_decide(&c, r.target_mode, r.min_events, r.margin);
    const char tc = class_of_decision(dec, r.target_mode);
    const double mine = r.target_mode == 0 ? c.on_score : c.off_score, other = r.target_mode == 0 ? c.off_score : c.on_score;
    const double tm = c.n_events > 0 ? (other - mine) / static_cast<double>(c.n_events) : NAN;
    char buf[96];
    if (std::isnan(tm))
        snprintf(buf, sizeof buf, "\ttc:A:%c\tac:A:%c\ttm:f:nan", tc, dec ? dec : 'P');
    else
        snprintf(buf, sizeof buf, "\ttc:A:%c\tac:A:%c\ttm:f:%.4f", tc, dec ? dec : 'P', tm);
    return buf;
}

struct Report {
    int64_t lines[3] = {0, 0, 0};  // E, F, R
    int64_t unmapped = 0, decided = 0, sum_ne = 0, samples_sent = 0;
    std::vector<double> tick_s;
    int64_t act_reads[3] = {0, 0, 0}, act_samples[3] = {0, 0, 0};  // --targets: A, U, P -- reads, samples sent plus held
    std::vector<int64_t> group_accepted;  // --by-name: accepted reads per best entry, the background last
    // quota > 0 (--quota): the named groups' lines gain quota=N closed_at=<tick whose credit closed the group, - for an open one>
    void print_groups(const std::vector<std::string> &names, int64_t quota = 0, const replay::Schedule *sch = nullptr) const {
        for (size_t g = 0; g < group_accepted.size(); ++g) {
            fprintf(stderr, "[realtime] group %s: accepted %ld reads", g < names.size() ? names[g].c_str() : "*", (long)group_accepted[g]);
            if (quota > 0 && g < names.size()) {
                const int64_t at = sch->closed_at(static_cast<int32_t>(g));
                fprintf(stderr, " quota=%ld closed_at=%s", (long)quota, at < 0 ? "-" : std::to_string(at).c_str());
            }
            fprintf(stderr, "\n");
        }
    }
    void print_targets() const {
        fprintf(stderr, "[realtime] targets: accepted (A) %ld reads, %ld samples\tunblocked (U) %ld reads, %ld samples\tproceeded (P) %ld reads, %ld samples (sent + held)\n",
                (long)act_reads[0], (long)act_samples[0], (long)act_reads[1], (long)act_samples[1], (long)act_reads[2], (long)act_samples[2]);
    }
    void print(const RealtimeOpt &r, const Channels &ch, double tick_signal_s) const {
        std::vector<double> t = tick_s;
        std::sort(t.begin(), t.end());
        const size_t n = t.size();
        double sum = 0;
        for (double x : t) sum += x;
        auto pct = [&](double p) { return n ? t[std::min(n - 1, static_cast<size_t>(p * static_cast<double>(n)))] : 0.0; };
        int64_t over = 0;
        for (double x : t) over += tick_signal_s > 0 && x > tick_signal_s;
        fprintf(stderr, "[realtime] reads: %ld\tlines: %ld early (E), %ld full (F), %ld at the end of the read (R)\tunmapped: %ld\n", (long)ch.reads,
                (long)lines[0], (long)lines[1], (long)lines[2], (long)unmapped);
        fprintf(stderr, "[realtime] mean query events at decision (ne): %.1f\n", decided ? static_cast<double>(sum_ne) / static_cast<double>(decided) : 0.0);
        fprintf(stderr, "[realtime] samples sent: %ld of %ld in the file (%.1f%% not sent)\n", (long)samples_sent, (long)ch.samples_in_file,
                ch.samples_in_file ? 100.0 * static_cast<double>(ch.samples_in_file - samples_sent) / static_cast<double>(ch.samples_in_file) : 0.0);
        fprintf(stderr, "[realtime] ticks: %zu of %ld samples on %d channels\ttick wall time: mean %.6f s, median %.6f s, p99 %.6f s, max %.6f s\n", n,
                (long)r.chunk_samples, r.channels, n ? sum / static_cast<double>(n) : 0.0, pct(0.5), pct(0.99), n ? t[n - 1] : 0.0);
        if (tick_signal_s > 0)
            fprintf(stderr, "[realtime] a tick is %.6f s of signal (%ld samples at %.0f Hz); %ld tick(s) took longer\n", tick_signal_s, (long)r.chunk_samples,
                    ch.sampling_rate, (long)over);
        else
            fprintf(stderr, "[realtime] the file gives no sampling rate: a tick's signal time is unknown\n");
    }
};

int realtime_run(int argc, char **argv, double t0) {
    RealtimeOpt r = parse_realtime_options(argc, argv);
    Opt &o = r.o;
    const bool with_truth = !r.truth.empty();
    const sfa::TruthTable truth = with_truth ? read_truth(r.truth, o.fasta) : sfa::TruthTable();
    sfa::Blow5Reader reader;
    if (!reader.open(o.blow5)) die(reader.error());
    detect_chemistry(reader, &o);
    if ((o.flag & F_RNA) && !(o.flag & F_INV) && !r.resweep)
        die("realtime: the file holds direct RNA: pass --rna --invert, or --rna --resweep (a session cannot extend a reversed query)");
    const Reference ref(o);
    Context ctx;
    // --spread: one context over the whole device list, the channels dealt over its devices; else the first device
    const int inited = r.spread ? sfa_init_devices(&ctx.c, &ref.view, o.flag, o.devices.data(), static_cast<int>(o.devices.size())) : sfa_init(&ctx.c, &ref.view, o.flag, o.devices[0]);
    if (inited != SFA_OK) die(std::string("accelerator init failed: ") + sfa_last_error());
    if (sfa_set_pore(ctx.c, o.pore_flag) != SFA_OK) die(sfa_last_error());
    sfa_session_t *se = nullptr;  // (freed with its context)
    if (sfa_session_create(ctx.c, r.channels, (r.resweep ? SFA_SESSION_RESWEEP : 0) | (r.spread ? SFA_SESSION_SPREAD : 0), &se) != SFA_OK) die(std::string("session: ") + sfa_last_error());
    if (sfa_session_raw_config(se, o.prefix, r.norm_events, o.query) != SFA_OK) die(std::string("session: ") + sfa_last_error());
    if (!r.recal_at.empty() || r.recal_at_end)
        if (sfa_session_raw_recalibrate(se, r.recal_at.data(), static_cast<int32_t>(r.recal_at.size()), r.recal_at_end ? SFA_RECAL_AT_END : 0) != SFA_OK)
            die(std::string("session: ") + sfa_last_error());
    if (r.candidates > 0 && sfa_session_candidates_config(se, r.candidates) != SFA_OK) die(std::string("session: ") + sfa_last_error());
    const bool targets = !r.targets.empty();
    int64_t reach_cols = 0;  // --lead: the on-target columns of the reach list; --group-lead: the labelled columns, which are the same columns
    std::vector<std::string> group_names;
    std::vector<sfa_target_t> t;  // (--truth reads both lists again at every decision)
    std::vector<sfa_group_target_t> gt;
    if (targets) {
        t = read_targets(r.targets, ref, r.by_name ? &gt : nullptr, r.by_name ? &group_names : nullptr);
        if (t.empty()) die("realtime: the targets file " + r.targets + " holds no interval");
        const bool group_reach = r.group_lead >= 0;  // --group-lead: mask and labels from the one list with the one lead
        std::vector<int8_t> strands;
        if (r.stranded || r.group_stranded) strands = read_strands(r.targets, r.stranded ? "--stranded" : "--group-stranded");
        if (r.lead >= 0 || group_reach) {  // --lead: the same intervals as reach targets; `t` stays what --truth reads
            std::vector<sfa_reach_target_t> rt(t.size());
            for (size_t k = 0; k < t.size(); ++k) {
                rt[k] = sfa_reach_target_t{};
                rt[k].contig = t[k].contig, rt[k].begin = t[k].begin, rt[k].end = t[k].end, rt[k].lead = group_reach ? r.group_lead : r.lead;
                rt[k].strand = strands.empty() ? 0 : strands[k];
            }
            if (sfa_session_targets_reach(se, rt.data(), static_cast<int32_t>(rt.size())) != SFA_OK) die(std::string("targets: ") + sfa_last_error());
            reach_cols = sfa_session_target_columns(se);
        } else if (sfa_session_targets(se, t.data(), static_cast<int32_t>(t.size())) != SFA_OK) {
            die(std::string("targets: ") + sfa_last_error());
        }
        if (group_reach) {  // the labels of the same list: which named target the read reaches first; `gt` stays what --truth reads
            std::vector<sfa_reach_group_target_t> rg(gt.size());
            for (size_t k = 0; k < gt.size(); ++k) {
                rg[k] = sfa_reach_group_target_t{};
                rg[k].contig = gt[k].contig, rg[k].begin = gt[k].begin, rg[k].end = gt[k].end, rg[k].lead = r.group_lead, rg[k].group = gt[k].group;
                rg[k].strand = strands.empty() ? 0 : strands[k];
            }
            if (sfa_session_target_groups_reach(se, rg.data(), static_cast<int32_t>(rg.size()), static_cast<int32_t>(group_names.size())) != SFA_OK)
                die(std::string("target groups: ") + sfa_last_error());
        } else if (r.by_name && sfa_session_target_groups(se, gt.data(), static_cast<int32_t>(gt.size()), static_cast<int32_t>(group_names.size())) != SFA_OK) {
            die(std::string("target groups: ") + sfa_last_error());
        }
    }
    int64_t base_cols = 0, open_cols = 0, cover_bases = 0, cover_intervals = 0;  // --depth-cap
    if (r.depth_cap > 0) {
        base_cols = sfa_session_target_columns(se);
        if (sfa_session_coverage_config(se, r.depth_cap) != SFA_OK) die(std::string("coverage: ") + sfa_last_error());
        open_cols = sfa_session_target_columns(se);
    }
    std::vector<sfa_group_cover_t> gcov(r.group_cap > 0 ? group_names.size() + 1 : 0);  // --group-cap: the groups' depth after every add
    std::vector<char> group_full(group_names.size(), 0);
    if (r.group_cap > 0) {
        if (sfa_session_group_coverage_config(se, r.group_cap) != SFA_OK) die(std::string("group coverage: ") + sfa_last_error());
        if (sfa_session_group_coverage(se, gcov.data(), static_cast<int32_t>(gcov.size())) != SFA_OK) die(std::string("group coverage: ") + sfa_last_error());
    }
    const bool use_open = r.quota > 0 || r.group_cap > 0;  // the tick's class call is sfa_session_open_classes; lines gain og
    std::vector<sfa_target_t> covered;  // of a tick: what its accepted reads add
    FILE *trace = nullptr;
    if (!r.trace.empty() && !(trace = fopen(r.trace.c_str(), "w"))) die("realtime: cannot write the trace to " + r.trace);
    if (o.verbosity >= 4)
        fprintf(stderr, "[realtime::%.3f] initialised: %d channels, %ld samples per tick, skip %d, norm %d, query %d, early at %d events and mapq %d\n", realtime() - t0,
                r.channels, (long)r.chunk_samples, o.prefix, r.norm_events, o.query, r.min_events, r.min_mapq);

    const int32_t C = r.channels;
    WorkerPool pool(o.threads);
    reader.start_prefault();
    ReadAhead ahead(reader, pool, 2 * static_cast<size_t>(C));
    Channels ch{ahead, std::vector<sfa::Blow5Record>(C)};
    replay::Schedule sch(C, r.chunk_samples, trace, targets);
    sfa::QuotaBook book(r.quota > 0 ? static_cast<int32_t>(group_names.size()) : 1, r.quota);
    if (r.quota > 0) sch.set_quota(&book, &group_names);
    const replay::Rule rule{r.min_events, r.min_mapq};
    Report rep;
    if (r.by_name) rep.group_accepted.assign(group_names.size() + 1, 0);
    std::vector<int32_t> lined_slot, head_of(r.by_name ? C : 0);
    std::vector<sfa_group_head_t> heads(r.by_name ? C : 0);

    double t_pin = 0;
    PinnedBuffer raw("sample");
    raw.grow(sizeof(int16_t) * (static_cast<size_t>(C) * static_cast<size_t>(r.chunk_samples) + 1), &t_pin);
    std::vector<int32_t> slot(C), decided_slot;
    std::vector<int64_t> raw_off(C + 1);
    std::vector<double> scaling(3 * static_cast<size_t>(C));
    std::vector<uint8_t> end(C);
    std::vector<sfa_result_t> rows(C);
    std::vector<sfa_session_raw_info_t> info(C);
    std::vector<char> reason(C), line(C), action(C);
    std::vector<sfa_class_t> cls(targets ? C : 0);
    std::vector<sfa_open_class_t> ocls(use_open ? C : 0);
    std::vector<int32_t> on_group(use_open ? C : 0);
    std::vector<int64_t> held;
    replay::TruthMarks marks;  // --truth: per entry of the tick
    std::vector<const sfa::TruthRecord *> truth_of(with_truth ? C : 0);
    std::vector<int64_t> len_now(with_truth ? C : 0);
    if (with_truth) marks.tt.assign(C, 'N'), marks.tv.assign(C, 'N');
    sfa::TruthAccount account;
    const int32_t n_targets = static_cast<int32_t>(t.size()), n_groups = static_cast<int32_t>(group_names.size());
    std::vector<uint64_t> span_a(C), span_b(C);
    std::vector<sfa_result_t> cand(r.candidates > 0 ? 4 * static_cast<size_t>(C) : 0);
    std::string text(4096, '\0');

    ahead.top_up();
    sch.start(ch);
    const auto start = std::chrono::steady_clock::now();
    while (sch.busy()) {
        if (r.pace && ch.sampling_rate > 0)  // (stderr timing only: nothing below reads a clock to decide anything)
            std::this_thread::sleep_until(start + std::chrono::duration<double>(static_cast<double>(sch.tick()) * static_cast<double>(r.chunk_samples) / ch.sampling_rate));
        const double a = realtime();
        ahead.top_up();  // decodes beside this tick's call
        const std::vector<replay::Entry> &es = sch.begin_tick();
        const int32_t n = static_cast<int32_t>(es.size());
        int16_t *dst = static_cast<int16_t *>(raw.data());
        raw_off[0] = 0;
        for (int32_t i = 0; i < n; ++i) {
            const replay::Entry &e = es[i];
            const sfa::Blow5Record &rec = ch.rec[e.channel];
            slot[i] = e.channel;
            if (e.count) memcpy(dst + raw_off[i], rec.raw.data() + e.first, sizeof(int16_t) * static_cast<size_t>(e.count));
            raw_off[i + 1] = raw_off[i] + e.count;
            scaling[3 * i] = rec.digitisation, scaling[3 * i + 1] = rec.offset, scaling[3 * i + 2] = rec.range;
            end[i] = e.end ? 1 : 0;
            rep.samples_sent += e.count;
        }
        if (sfa_session_extend_raw(se, slot.data(), dst, raw_off.data(), scaling.data(), end.data(), n, rows.data(), info.data()) != SFA_OK)
            die(std::string("tick ") + std::to_string(sch.tick()) + ": " + sfa_last_error());
        decided_slot.clear();
        if (use_open && n > 0) {  // the tick's classes under the groups open at its start (the book changes in end_tick only; no book: every group)
            if (sfa_session_open_classes(se, slot.data(), n, r.quota > 0 ? book.open() : nullptr, r.quota > 0 ? book.n_words() : 0, ocls.data()) != SFA_OK) die(std::string("open classes: ") + sfa_last_error());
            for (int32_t i = 0; i < n; ++i) cls[i] = ocls[i].cls, on_group[i] = ocls[i].on_group;
        } else if (targets && n > 0 && sfa_session_classes(se, slot.data(), n, cls.data()) != SFA_OK) {
            die(std::string("classes: ") + sfa_last_error());
        }
        for (int32_t i = 0; i < n; ++i) {
            replay::Status s;
            s.calibrated = info[i].status & 1, s.full = info[i].status & 2, s.ended = info[i].status & 4, s.poisoned = info[i].status & 8;
            s.mapped = rows[i].valid && rows[i].rid >= 0;
            s.q_events = info[i].q_events;
            s.mapq = rows[i].mapq;
            if (targets) {
                const char dec = static_cast<char>(sfa_target_decide(&cls[i], r.target_mode, r.min_events, r.margin));
                reason[i] = replay::decide_targets(s, dec);
                action[i] = reason[i] ? replay::action_of(reason[i], dec) : 0;
            } else {
                reason[i] = replay::decide(rule, s);
            }
            line[i] = reason[i] && s.mapped;
            if (reason[i]) decided_slot.push_back(slot[i]);
            if (reason[i] && with_truth) {  // one look-up per read, at its decision
                truth_of[i] = truth.find(ch.rec[slot[i]].read_id);
                marks.tt[i] = sfa::truth_class_of(truth_of[i], t.data(), n_targets);
                marks.tv[i] = sfa::truth_verdict(class_of_decision(sfa_target_decide(&cls[i], r.target_mode, r.min_events, r.margin), r.target_mode), marks.tt[i]);
                len_now[i] = sch.length(slot[i]);
            }
        }
        const int32_t nd = static_cast<int32_t>(decided_slot.size());
        if (nd > 0) {
            if (sfa_session_query_span(se, decided_slot.data(), nd, span_a.data(), span_b.data()) != SFA_OK) die(std::string("query span: ") + sfa_last_error());
            // the candidates of every channel decided in this tick, in one call and before the reset
            if (r.candidates > 0 && sfa_session_candidates(se, decided_slot.data(), nd, cand.data()) != SFA_OK) die(std::string("candidates: ") + sfa_last_error());
            if (r.by_name) {  // one call over the channels that print a line in this tick, before the reset
                lined_slot.clear();
                for (int32_t i = 0; i < n; ++i) {
                    head_of[i] = reason[i] && line[i] ? static_cast<int32_t>(lined_slot.size()) : -1;
                    if (head_of[i] >= 0) lined_slot.push_back(slot[i]);
                }
                if (!lined_slot.empty() && sfa_session_group_bests(se, lined_slot.data(), static_cast<int32_t>(lined_slot.size()), nullptr, heads.data()) != SFA_OK)
                    die(std::string("group bests: ") + sfa_last_error());
            }
            for (int32_t i = 0, d = 0; i < n; ++i) {  // ascending channels
                if (!reason[i]) continue;
                const int32_t k = d++;
                ++rep.decided;
                rep.sum_ne += info[i].q_events;
                if (!line[i]) {
                    ++rep.unmapped;
                    continue;
                }
                const sfa::Blow5Record &rec = ch.rec[slot[i]];
                std::string tail = targets ? target_tags(cls[i], r) : std::string();
                if (r.by_name) {
                    const sfa_group_head_t &h = heads[head_of[i]];
                    tail += replay::group_tags(h.best, h.second, h.best_score, h.second_score, h.n_events, group_names);
                    if (action[i] == 'A' && h.best >= 0) ++rep.group_accepted[h.best];
                }
                if (use_open) tail += replay::quota_tags(on_group[i], group_names);
                if (with_truth) {
                    tail += replay::truth_tags(marks.tt[i], marks.tv[i]);
                    if (r.by_name) {  // the line's tg names the head's best entry, the background for none
                        const sfa::TruthRecord *w = truth_of[i];
                        const int32_t best = heads[head_of[i]].best, said = best >= 0 && best < n_groups ? best : n_groups;
                        const int32_t true_group = w ? sfa::truth_group(gt.data(), static_cast<int32_t>(gt.size()), n_groups, w->contig, w->begin, w->end) : -1;
                        const char gv = sfa::truth_group_verdict(said, true_group);
                        tail += replay::truth_group_tags(true_group, gv, group_names);
                        account.note_group(gv);
                    }
                }
                // the primary, then the channel's valid candidates, best first: same span, same tags
                for (int32_t m = 0; m <= r.candidates; ++m) {
                    const sfa_result_t &w = m == 0 ? rows[i] : cand[4 * static_cast<size_t>(k) + (m - 1)];
                    if (m > 0 && !(w.valid && w.rid >= 0)) continue;
                    // query_size as dtw passes it: last query event - first (src/sigfish.c:801-807)
                    int len = sfa_paf_row_ex(&text[0], text.size(), &w, rec.read_id.c_str(), ref.contigs[w.rid].name.c_str(), span_a[k], span_b[k],
                                             static_cast<uint64_t>(info[i].q_events - 1), rec.raw.size(), static_cast<uint64_t>(ref.seq_len[w.rid]), m == 0 ? 'P' : 'S');
                    if (len > 0) {
                        const int more = snprintf(&text[len - 1], text.size() - static_cast<size_t>(len - 1), "\tne:i:%ld\tns:i:%ld\tdc:A:%c%s\n", (long)info[i].q_events,
                                                  (long)info[i].n_samples, reason[i], tail.c_str());
                        len = (more < 0 || static_cast<size_t>(len - 1 + more) >= text.size()) ? -1 : len - 1 + more;
                    }
                    if (len < 0) die("PAF line too long");
                    fwrite(text.data(), 1, static_cast<size_t>(len), stdout);
                }
                ++rep.lines[reason[i] == 'E' ? 0 : reason[i] == 'F' ? 1 : 2];
                // --depth-cap: an accepted read covers the target interval of its line (a row of one column has none)
                if ((r.depth_cap > 0 || r.group_cap > 0) && action[i] == 'A' && rows[i].pos_st >= 0 && rows[i].pos_end > rows[i].pos_st) covered.push_back(sfa_target_t{rows[i].rid, rows[i].pos_st, rows[i].pos_end});
            }
            fflush(stdout);  // a line is out at the moment of its decision
            if (sfa_session_reset(se, decided_slot.data(), nd) != SFA_OK) die(std::string("reset: ") + sfa_last_error());
        }
        if (targets) {
            std::vector<int64_t> sent_now(n);
            for (int32_t i = 0; i < n; ++i) sent_now[i] = sch.sent(slot[i]);
            const int64_t tick_now = sch.tick();
            sch.end_tick(reason, line, ch, &action, &held, r.quota > 0 ? &on_group : nullptr, with_truth ? &marks : nullptr);
            if (!covered.empty()) {  // one call for the tick; the new mask holds from the next tick on
                if (sfa_session_coverage_add(se, covered.data(), static_cast<int32_t>(covered.size()), &open_cols) != SFA_OK) die(std::string("coverage: ") + sfa_last_error());
                if (trace) fprintf(trace, "tick %ld cover n=%zu open=%ld\n", (long)tick_now, covered.size(), (long)open_cols);
                cover_intervals += static_cast<int64_t>(covered.size());
                for (const sfa_target_t &iv : covered) cover_bases += iv.end - iv.begin;
                covered.clear();
                if (r.group_cap > 0) {  // how deep every group is now; a group whose every column is capped is reported once
                    if (sfa_session_group_coverage(se, gcov.data(), static_cast<int32_t>(gcov.size())) != SFA_OK) die(std::string("group coverage: ") + sfa_last_error());
                    for (size_t g = 0; g < group_names.size(); ++g)
                        if (!group_full[g] && replay::group_is_full(gcov[g].columns, gcov[g].capped)) {
                            group_full[g] = 1;
                            if (trace) fprintf(trace, "tick %ld full group=%s\n", (long)tick_now, group_names[g].c_str());
                        }
                }
            }
            for (int32_t i = 0; i < n; ++i) {
                if (!reason[i]) continue;
                const int a = action[i] == 'A' ? 0 : action[i] == 'U' ? 1 : 2;
                ++rep.act_reads[a];
                rep.act_samples[a] += sent_now[i] + held[i];
                if (with_truth) {
                    const sfa::TruthRecord *w = truth_of[i];
                    account.note(marks.tt[i], w && sfa::truth_edge(t.data(), n_targets, w->contig, w->begin, w->end), action[i], marks.tv[i], sent_now[i], held[i], len_now[i]);
                }
            }
        } else {
            sch.end_tick(reason, line, ch);
        }
        rep.tick_s.push_back(realtime() - a);
    }
    if (trace) fclose(trace);
    if (targets) rep.print_targets();
    if (r.lead >= 0) fprintf(stderr, "[realtime] reach: lead %d%s\ton-target columns: %ld\n", r.lead, r.stranded ? ", stranded" : "", (long)reach_cols);
    if (r.group_lead >= 0) fputs(replay::reach_group_line(r.group_lead, r.group_stranded, reach_cols).c_str(), stderr);
    if (r.depth_cap > 0)
        fprintf(stderr, "[realtime] coverage: cap %d\t%ld intervals, %ld bases added\topen target columns at the end: %ld of %ld\n", r.depth_cap, (long)cover_intervals,
                (long)cover_bases, (long)open_cols, (long)base_cols);
    if (r.by_name) rep.print_groups(group_names, r.quota, &sch);
    if (r.group_cap > 0) {
        fprintf(stderr, "[realtime] group cap %d\t%ld intervals, %ld bases added\n", r.group_cap, (long)cover_intervals, (long)cover_bases);
        for (size_t g = 0; g < group_names.size(); ++g) fputs(replay::group_cover_line(group_names[g], gcov[g].columns, gcov[g].capped, gcov[g].depth_sum).c_str(), stderr);
    }
    if (o.verbosity >= 3) rep.print(r, ch, ch.sampling_rate > 0 ? static_cast<double>(r.chunk_samples) / ch.sampling_rate : 0.0);
    if (with_truth) fputs(account.format(r.by_name).c_str(), stderr);
    return 0;
}

}  // namespace
}  // namespace cli

int realtime_main(int argc, char **argv) {
    using namespace cli;
    const double t0 = realtime();
    try {
        return realtime_run(argc, argv, t0);
    } catch (const Fatal &e) {  // the helper that decodes ahead has been joined by the unwinding
        fflush(stdout);
        fprintf(stderr, "[sigfish-amd] ERROR: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
