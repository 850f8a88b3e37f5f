// The schedule of `sigfish-amd realtime --truth` (sigfish_amd/csrc/cli/replay.hpp: a `verdict` line behind every `decide` line)
// as a stand-alone host program with a scripted stub in place of the session; tests/test_replay_truth_cpu.py builds it under
// ASan + UBSan, drives the Python twin (sigfish_amd/realtime.py: Schedule) with the same script and compares the traces line for
// line.
//   stdin: <channels> <chunk> <truth 0|1> <quota, 0: none> <n reads>, then per read: <length> <decide once this many samples are
//          sent> <A|U|P> <decided class T|O|N> <true class T|O|N>
//   A read decides 'E' with its action once that many samples are out, else 'R' with 'P' at its end.  With a quota every read is of
//   one group, `g`, so that `close` lines meet `verdict` lines.  The verdict is truth_rules.hpp's; the program also prints the
//   truth tags of every decided read (`tags ...`) and ends with the account's `truth:` lines.
#include <stdio.h>

#include <string>
#include <vector>

#include "cli/replay.hpp"
#include "truth_rules.hpp"

struct Source {
    std::vector<long> len;
    size_t next = 0;
    bool take(int32_t, int64_t *n) {
        if (next >= len.size()) return false;
        *n = len[next++];
        return true;
    }
};

int main() {
    int channels, with_truth, n_reads;
    long chunk, quota;
    if (scanf("%d %ld %d %ld %d", &channels, &chunk, &with_truth, &quota, &n_reads) != 5 || n_reads < 0) return 2;
    Source src;
    std::vector<long> at(n_reads);
    std::vector<char> act(n_reads), tc(n_reads), tt(n_reads);
    src.len.resize(n_reads);
    for (int i = 0; i < n_reads; ++i)
        if (scanf("%ld %ld %c %c %c", &src.len[i], &at[i], &act[i], &tc[i], &tt[i]) != 5) return 2;
    const std::vector<std::string> names = {"g"};
    sfa::QuotaBook book(1, quota);
    cli::replay::Schedule sch(channels, chunk, stdout, true);
    if (quota > 0) sch.set_quota(&book, &names);
    sch.start(src);
    std::vector<int64_t> held;
    sfa::TruthAccount account;
    while (sch.busy()) {
        const std::vector<cli::replay::Entry> &es = sch.begin_tick();
        std::vector<char> reason(es.size()), line(es.size()), action(es.size());
        std::vector<int32_t> on_group(es.size(), 0);
        std::vector<int64_t> sent(es.size());
        cli::replay::TruthMarks marks;
        marks.tt.assign(es.size(), 'N'), marks.tv.assign(es.size(), 'N');
        for (size_t i = 0; i < es.size(); ++i) {
            sent[i] = es[i].first + es[i].count;
            reason[i] = sent[i] >= at[es[i].read] ? 'E' : (es[i].end ? 'R' : 0);
            line[i] = reason[i] == 'E';
            action[i] = reason[i] ? cli::replay::action_of(reason[i], act[es[i].read]) : 0;
            if (!reason[i]) continue;
            marks.tt[i] = tt[es[i].read];
            marks.tv[i] = sfa::truth_verdict(reason[i] == 'E' ? tc[es[i].read] : 'N', marks.tt[i]);
        }
        const std::vector<cli::replay::Entry> now = es;  // (end_tick keeps the entries; a copy for the lines below)
        sch.end_tick(reason, line, src, &action, &held, quota > 0 ? &on_group : nullptr, with_truth ? &marks : nullptr);
        for (size_t i = 0; i < now.size(); ++i) {
            if (!reason[i]) continue;
            account.note(marks.tt[i], false, action[i], marks.tv[i], sent[i], held[i], src.len[now[i].read]);
            if (with_truth) printf("tags read=%ld %s\n", (long)now[i].read, cli::replay::truth_tags(marks.tt[i], marks.tv[i]).c_str());
        }
    }
    printf("end tick=%ld\n", (long)sch.tick());
    if (with_truth) fputs(account.format(false).c_str(), stdout);
    return 0;
}
