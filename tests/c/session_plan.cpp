// The host rules of a session call (sigfish_amd/csrc/session_plan.hpp, the header sfa_session.hip plans with) as a stand-alone
// host program.  It reads requests from stdin and prints what the header answers; tests/test_session_plan_cpu.py compares every
// line with the Python restatements (tests/session_waves.py: plan_call, tests/autostart_oracle.py: points_between).
//   plan <n_jobs> <n>, then n lines "<slot> <chunk events> <events held> <poisoned>"
//     -> "call <launches> <new events> <call_slot x n>", per launch "launch <n_cls> <n_tasks> <groups> <entries>",
//        "cls <R> <lanes> <first> <group_base> <n_groups> <task_base>", "group <g_qlen> <w_entry x 4>",
//        "entry <call> <slot> <len> <total> <off>"
//   auto <have> <after> <ended_now> <every> <max_samples> <k_done> <settled>
//     -> "auto <n0> <n_periodic> <n_final> <k_after> <final_now> <pending>"
#include <cstdio>
#include <cstring>

#include "session_plan.hpp"

static int plan(int n_jobs, int n) {
    std::vector<int32_t> slot(n);
    std::vector<sfa::Chunk> ch(n);
    std::vector<int64_t> held;
    std::vector<uint8_t> poison;
    int64_t off = 0;
    for (int i = 0; i < n; ++i) {
        long long len = 0, have = 0;
        int bad = 0;
        if (scanf("%d %lld %lld %d", &slot[i], &len, &have, &bad) != 4 || slot[i] < 0 || len < 0 || have < 0) return 2;
        if (static_cast<size_t>(slot[i]) >= held.size()) held.resize(slot[i] + 1, 0), poison.resize(slot[i] + 1, 0);
        held[slot[i]] = have;
        poison[slot[i]] = bad ? 1 : 0;
        ch[i] = sfa::Chunk{off, len};  // back to back, as sfa_session_extend lays them out
        off += len;
    }
    std::vector<sfa::Launch> launches;
    std::vector<int32_t> call_slot;
    int64_t new_events = -1;
    sfa::plan_session_call(ch.data(), slot.data(), held.data(), poison.data(), n, n_jobs, &launches, &call_slot, &new_events);
    printf("call %zu %lld", launches.size(), static_cast<long long>(new_events));
    for (int32_t cs : call_slot) printf(" %d", cs);
    printf("\n");
    for (const sfa::Launch &l : launches) {
        if (l.n_cls > sfa::kSessionMaxClasses || l.w_entry.size() != 4 * l.g_qlen.size()) return 3;
        printf("launch %d %d %zu %zu\n", l.n_cls, l.n_tasks, l.g_qlen.size(), l.k_off.size());
        for (int c = 0; c < l.n_cls; ++c)
            printf("cls %d %d %d %d %d %d\n", l.cls[c].R, l.cls[c].lanes, l.cls[c].first, l.cls[c].group_base, l.cls[c].n_groups, l.cls[c].task_base);
        for (size_t g = 0; g < l.g_qlen.size(); ++g)
            printf("group %d %d %d %d %d\n", l.g_qlen[g], l.w_entry[4 * g], l.w_entry[4 * g + 1], l.w_entry[4 * g + 2], l.w_entry[4 * g + 3]);
        for (size_t e = 0; e < l.k_off.size(); ++e)
            printf("entry %d %d %d %d %lld\n", l.k_call[e], l.k_slot[e], l.k_len[e], l.k_total[e], static_cast<long long>(l.k_off[e]));
    }
    return 0;
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "plan")) {
            int n_jobs = 0, n = 0;
            if (scanf("%d %d", &n_jobs, &n) != 2 || n_jobs <= 0 || n < 0) return 2;
            if (int rc = plan(n_jobs, n)) return rc;
        } else if (!strcmp(what, "auto")) {
            long long have = 0, after = 0;
            int ended = 0, every = 0, max_samples = 0, k_done = 0, settled = 0;
            if (scanf("%lld %lld %d %d %d %d %d", &have, &after, &ended, &every, &max_samples, &k_done, &settled) != 7) return 2;
            const sfa::AutoPoints p = sfa::auto_points(have, after, ended != 0, every, max_samples, k_done, settled != 0);
            printf("auto %d %d %d %d %d %d\n", p.n0, p.n_periodic, p.n_final, p.k_after, p.final_now ? 1 : 0, p.pending ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
