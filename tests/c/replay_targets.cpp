// The schedule of `sigfish-amd realtime` with targets (sigfish_amd/csrc/cli/replay.hpp: hold ticks, channels freed by an unblock)
// as a stand-alone host program with a scripted stub in place of the session; tests/test_session_targets_cpu.py drives the Python
// twin (sigfish_amd/realtime.py: Schedule) with the same script and compares the traces line for line.
//   stdin: <channels> <chunk> <targets 0|1> <n reads>, then per read: <length> <decide once this many samples are sent> <A|U|P>
//   A read decides 'E' with its action once that many samples are out, else 'R' with 'P' at its end; the trace goes to stdout.
#include <stdio.h>

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

int main() {
    int channels, targets, n_reads;
    long chunk;
    if (scanf("%d %ld %d %d", &channels, &chunk, &targets, &n_reads) != 4) return 2;
    Source src;
    std::vector<long> at(n_reads);
    std::vector<char> act(n_reads);
    src.len.resize(n_reads);
    for (int i = 0; i < n_reads; ++i)
        if (scanf("%ld %ld %c", &src.len[i], &at[i], &act[i]) != 3) return 2;
    cli::replay::Schedule sch(channels, chunk, stdout, targets != 0);
    sch.start(src);
    std::vector<int64_t> held;
    long total_held = 0;
    while (sch.busy()) {
        const std::vector<cli::replay::Entry> &es = sch.begin_tick();
        std::vector<char> reason(es.size()), line(es.size()), action(es.size());
        for (size_t i = 0; i < es.size(); ++i) {
            const long sent = es[i].first + es[i].count;
            reason[i] = sent >= at[es[i].read] ? 'E' : (es[i].end ? 'R' : 0);
            line[i] = reason[i] == 'E';
            action[i] = reason[i] ? cli::replay::action_of(reason[i], act[es[i].read]) : 0;
        }
        if (targets) {
            sch.end_tick(reason, line, src, &action, &held);
            for (int64_t h : held) total_held += h;
        } else {
            sch.end_tick(reason, line, src);
        }
    }
    printf("end tick=%ld held=%ld\n", (long)sch.tick(), total_held);
    return 0;
}
