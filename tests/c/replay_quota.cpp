// The schedule of `sigfish-amd realtime --quota` (sigfish_amd/csrc/cli/replay.hpp: accepted reads credited per group, groups closed
// from the next tick on) as a stand-alone host program with a scripted stub in place of the session; tests/test_session_quota_cpu.py
// builds it under ASan + UBSan, drives the Python twin (sigfish_amd/realtime.py: Schedule) with the same script and compares the
// traces line for line.
//   stdin: <channels> <chunk> <quota> <n groups> <name per group> <n reads>, then per read: <length> <decide once this many samples
//          are sent> <group, -1: the background> <line 0|1>
//   The stub answers as the open-class call would: a read decides 'E' once that many samples are out -- accepted ('A', on_group its
//   group) when its group was open WHEN THE TICK BEGAN, else unblocked ('U', on_group -1) -- or 'R' with 'P' at its end.  The program
//   checks the schedule's properties itself: a group closes in the tick in which its count reaches the quota, is credited no read in
//   any later tick, and its count is the quota plus what its closing tick accepted beyond it.  The trace goes to stdout.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "cli/replay.hpp"

struct Source {
    std::vector<long> len;
    size_t next = 0;
    bool take(int32_t, int64_t *n) {
        if (next >= len.size()) return false;
        *n = len[next++];
        return true;
    }
};

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                 \
        }                                                            \
    } while (0)

int main() {
    int channels, n_groups, n_reads;
    long chunk, quota;
    if (scanf("%d %ld %ld %d", &channels, &chunk, &quota, &n_groups) != 4 || n_groups < 1 || n_groups > sfa::kGroupMax) return 2;
    std::vector<std::string> names(n_groups);
    for (std::string &s : names) {
        char buf[64];
        if (scanf("%63s", buf) != 1) return 2;
        s = buf;
    }
    if (scanf("%d", &n_reads) != 1 || n_reads < 0) return 2;
    Source src;
    std::vector<long> at(n_reads);
    std::vector<int> group(n_reads), lined(n_reads);
    src.len.resize(n_reads);
    for (int i = 0; i < n_reads; ++i)
        if (scanf("%ld %ld %d %d", &src.len[i], &at[i], &group[i], &lined[i]) != 4 || group[i] >= n_groups) return 2;
    sfa::QuotaBook book(n_groups, quota);
    cli::replay::Schedule sch(channels, chunk, stdout, true);
    sch.set_quota(&book, &names);
    sch.start(src);
    std::vector<int64_t> held;
    std::vector<long> credited(n_groups, 0), in_closing_tick(n_groups, 0);
    while (sch.busy()) {
        const int64_t tick = sch.tick();
        const std::vector<cli::replay::Entry> &es = sch.begin_tick();
        std::vector<char> open(n_groups);
        for (int g = 0; g < n_groups; ++g) open[g] = book.is_open(g);  // the bitmap the tick's call would carry
        std::vector<char> reason(es.size()), line(es.size()), action(es.size());
        std::vector<int32_t> on_group(es.size(), -1);
        for (size_t i = 0; i < es.size(); ++i) {
            const long sent = es[i].first + es[i].count;
            const int g = group[es[i].read];
            reason[i] = sent >= at[es[i].read] ? 'E' : (es[i].end ? 'R' : 0);
            line[i] = reason[i] == 'E' && lined[es[i].read];
            const bool on = g >= 0 && open[g];
            on_group[i] = on ? g : -1;
            action[i] = reason[i] ? cli::replay::action_of(reason[i], on ? 'A' : 'U') : 0;
            if (action[i] == 'A' && line[i]) {
                CHECK(sch.closed_at(g) < 0);  // no credit in a tick after the closing one
                ++credited[g];
                if (quota > 0 && credited[g] >= quota) ++in_closing_tick[g];
            }
        }
        sch.end_tick(reason, line, src, &action, &held, &on_group);
        for (int g = 0; g < n_groups; ++g) {
            CHECK(book.accepted(g) == credited[g]);
            CHECK((sch.closed_at(g) >= 0) == !book.is_open(g) && (quota > 0 && credited[g] >= quota) == !book.is_open(g));
            if (open[g] && !book.is_open(g)) CHECK(sch.closed_at(g) == tick && credited[g] == quota + in_closing_tick[g] - 1);
        }
    }
    printf("end tick=%ld", (long)sch.tick());
    for (int g = 0; g < n_groups; ++g) printf(" %s=%ld@%ld", names[g].c_str(), (long)book.accepted(g), (long)sch.closed_at(g));
    printf("\n");
    return 0;
}
