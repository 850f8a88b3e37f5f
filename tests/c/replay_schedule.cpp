// replay_schedule.cpp -- the schedule of `sigfish-amd realtime` (sigfish_amd/csrc/cli/replay.hpp) driven by a stub in place of
// the session: a scripted table says at which chunk of a read the stub reports "early", "full" or "poisoned" and whether the row
// is mapped.  Host only, built under ASan + UBSan by tests/test_realtime_cpu.py, which runs the same table through the Python
// twin (sigfish_amd/realtime.py) and compares the traces line for line.
//
// The table (tests/test_realtime_cpu.py restates it): S = 8; read i has lens[i % 6] samples of {0, 1, S - 1, S, S + 1, 3 S};
// timing (i + i / 6) % 3: 0 decided at its first chunk, 1 at its last (chunk len / S + 1), 2 never (it runs to its end);
// a decision is early for even i, full for odd i; the row is mapped unless i % 4 == 3; reads 10 and 15 (timing 2) are poisoned
// at their first chunk.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cli/replay.hpp"

using cli::replay::Entry;
using cli::replay::Rule;
using cli::replay::Schedule;
using cli::replay::Status;

namespace {

constexpr int64_t S = 8;

struct Script {
    int64_t len;
    int64_t k;  // the chunk at which the stub fires (0: never)
    bool early, mapped, poison;
};

Script script_for(int64_t i) {
    const int64_t lens[6] = {0, 1, S - 1, S, S + 1, 3 * S};
    Script s;
    s.len = lens[i % 6];
    const int timing = static_cast<int>((i + i / 6) % 3);
    s.k = timing == 0 ? 1 : timing == 1 ? s.len / S + 1 : 0;
    s.early = i % 2 == 0;
    s.mapped = i % 4 != 3;
    s.poison = timing == 2 && (i == 10 || i == 15);
    return s;
}

int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++failures;                                    \
            fprintf(stderr, "FAILED %s: ", #cond);         \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

struct Source {
    int64_t n_reads, next = 0;
    bool take(int32_t, int64_t *len) {
        if (next >= n_reads) return false;
        *len = script_for(next++).len;
        return true;
    }
};

void run_case(int32_t C, int64_t N) {
    printf("case C=%d reads=%ld\n", C, (long)N);
    fflush(stdout);
    Source src{N};
    Schedule sch(C, S, stdout);
    const Rule rule{30, 20};
    std::vector<int64_t> sent(N, 0), chunks(N, 0), take_tick(N, -1), channel(N, -1), decided_at(N, -1);  // take_tick -1: at setup
    std::vector<char> saw_end(N, 0);
    std::vector<int64_t> on(C, -1);  // our own book of the channels, from what the schedule hands out
    sch.start(src);
    CHECK(sch.reads_taken() == (N < C ? N : C), "setup took %ld reads", (long)sch.reads_taken());
    int64_t taken = sch.reads_taken();
    for (int64_t r = 0; r < taken; ++r) on[r] = r, channel[r] = r;  // read i on channel i
    int64_t total_chunks = 0;
    for (int64_t i = 0; i < N; ++i) total_chunks += script_for(i).len / S + 1;
    while (sch.busy()) {
        const int64_t t = sch.tick();
        if (t > total_chunks + N) {  // every tick with a busy channel sends a chunk, and there are only so many
            CHECK(false, "C=%d reads=%ld does not terminate", C, (long)N);
            return;
        }
        const std::vector<Entry> es = sch.begin_tick();
        int32_t busy = 0;
        for (int32_t c = 0; c < C; ++c) busy += on[c] >= 0;
        CHECK(static_cast<int32_t>(es.size()) == busy, "tick %ld: %zu entries for %d busy channels", (long)t, es.size(), busy);
        std::vector<char> reason(es.size(), 0), line(es.size(), 0);
        for (size_t i = 0; i < es.size(); ++i) {
            const Entry &e = es[i];
            CHECK(i == 0 || es[i - 1].channel < e.channel, "tick %ld: channels not ascending", (long)t);
            CHECK(e.read >= 0 && e.read < N && on[e.channel] == e.read, "tick %ld: read %ld is not on channel %d", (long)t, (long)e.read, e.channel);
            if (e.read < 0 || e.read >= N) return;
            const Script s = script_for(e.read);
            CHECK(decided_at[e.read] < 0, "read %ld sends after its decision", (long)e.read);
            CHECK(!saw_end[e.read], "read %ld sends after its end", (long)e.read);
            CHECK(e.first == sent[e.read], "read %ld: chunk starts at %ld, %ld were sent", (long)e.read, (long)e.first, (long)sent[e.read]);
            CHECK(e.count >= 0 && e.count <= S && e.first + e.count <= s.len, "read %ld: chunk of %ld", (long)e.read, (long)e.count);
            CHECK(e.count == (s.len - e.first < S ? s.len - e.first : S) && e.end == (e.count < S), "read %ld: chunk of %ld, end %d", (long)e.read, (long)e.count, e.end);
            if (chunks[e.read] == 0)
                CHECK(t == take_tick[e.read] + 1 && e.channel == channel[e.read], "read %ld taken at tick %ld by channel %ld first sends at tick %ld on channel %d",
                      (long)e.read, (long)take_tick[e.read], (long)channel[e.read], (long)t, e.channel);
            sent[e.read] += e.count;
            saw_end[e.read] = e.end;
            const int64_t j = ++chunks[e.read];
            // the stub session
            Status st;
            st.ended = e.end;
            st.mapped = s.mapped;
            if (s.poison) {
                st.poisoned = true;
                st.mapped = false;
            } else if (s.k && j == s.k) {
                if (s.early) st.calibrated = true, st.q_events = 100, st.mapped = true, st.mapq = 60;
                else st.full = true;
            }
            reason[i] = cli::replay::decide(rule, st);
            line[i] = reason[i] && st.mapped;
            if (reason[i]) decided_at[e.read] = t, on[e.channel] = -1;
        }
        const int64_t before = sch.reads_taken();
        sch.end_tick(reason, line, src);
        // freed channels took the lowest unread records, lowest channel first, and send from the next tick on
        int64_t nxt = before;
        for (size_t i = 0; i < es.size(); ++i)
            if (reason[i] && nxt < N) on[es[i].channel] = nxt, channel[nxt] = es[i].channel, ++nxt;
        CHECK(sch.reads_taken() == nxt, "tick %ld: %ld reads taken, expected %ld", (long)t, (long)sch.reads_taken(), (long)nxt);
        for (int64_t r = before; r < nxt; ++r) take_tick[r] = t;  // (its first chunk must go out at t + 1: checked at that send)
        CHECK(sch.tick() == t + 1, "tick did not advance");
    }
    printf("end ticks=%ld reads=%ld\n", (long)sch.tick(), (long)sch.reads_taken());
    CHECK(sch.reads_taken() == N, "%ld of %ld reads taken", (long)sch.reads_taken(), (long)N);
    for (int64_t r = 0; r < N; ++r) {
        const Script s = script_for(r);
        CHECK(decided_at[r] >= 0, "read %ld was never decided", (long)r);
        const int64_t want_chunks = s.poison ? 1 : s.k ? s.k : s.len / S + 1;
        CHECK(chunks[r] == want_chunks, "read %ld: %ld chunks, expected %ld", (long)r, (long)chunks[r], (long)want_chunks);
        if (!s.k && !s.poison) CHECK(sent[r] == s.len && saw_end[r], "read %ld ran to its end with %ld of %ld samples", (long)r, (long)sent[r], (long)s.len);
    }
}

}  // namespace

int main() {
    const int32_t Cs[3] = {1, 3, 8};
    const int64_t Ns[4] = {0, 1, 7, 20};
    int cases = 0;
    for (int32_t C : Cs)
        for (int64_t N : Ns) {
            run_case(C, N);
            ++cases;
        }
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
