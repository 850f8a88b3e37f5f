// The entry selection of a session's query calls (sigfish_amd/csrc/session_query.hpp, the header query_run of
// sfa_session_targets.hip selects and scatters with) as a stand-alone host program.  It reads requests from stdin and prints what
// the header answers; tests/test_session_query_cpu.py compares every line with its own arithmetic.
//   live <n_slots> <n>, then n_slots pairs "<poisoned> <events held>", then the n slots of the call
//     -> "live <m> <live x m>"       the caller's indices of the entries that launch
//        "slots <slot x m>"          the slot list as it is uploaded: launched entry k is slot[live[k]]
//        "out <record x n>"          the caller's records: -1, the "none" record, or 1000 * k + slot for launched entry k
//   fit <m> <parts>
//     -> "fit <0 | 1>"               m x parts blocks are what a launch takes
#include <cstdio>
#include <cstring>

#include "session_query.hpp"

static int live(int n_slots, int n) {
    std::vector<uint8_t> poison(n_slots);
    std::vector<int64_t> len(n_slots);
    std::vector<int32_t> slot(n);
    for (int sl = 0; sl < n_slots; ++sl) {
        int bad = 0;
        long long have = 0;
        if (scanf("%d %lld", &bad, &have) != 2 || have < 0) return 2;
        poison[sl] = bad ? 1 : 0;
        len[sl] = have;
    }
    for (int i = 0; i < n; ++i)
        if (scanf("%d", &slot[i]) != 1 || slot[i] < 0 || slot[i] >= n_slots) return 2;
    std::vector<int32_t> lv(3, 77);  // (what an earlier call left is cleared)
    sfa::query_live_entries(slot.data(), n, poison.data(), len.data(), &lv);
    const int m = static_cast<int>(lv.size());
    std::vector<int32_t> hs(m, -7);  // the slot list, and the records scattered behind the "none" records: the header's, as query_run calls them
    sfa::query_live_slots(slot.data(), lv, hs.data());
    std::vector<int32_t> out(n, -1);
    sfa::query_scatter(slot.data(), lv, [&](int32_t k, int32_t i, int32_t sl) { out[i] = 1000 * k + sl; });
    printf("live %d", m);
    for (int32_t i : lv) printf(" %d", i);
    printf("\nslots");
    for (int32_t sl : hs) printf(" %d", sl);
    printf("\nout");
    for (int32_t r : out) printf(" %d", r);
    printf("\n");
    return 0;
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "live")) {
            int n_slots = 0, n = 0;
            if (scanf("%d %d", &n_slots, &n) != 2 || n_slots <= 0 || n < 0) return 2;
            if (int rc = live(n_slots, n)) return rc;
        } else if (!strcmp(what, "fit")) {
            int m = 0, parts = 0;
            if (scanf("%d %d", &m, &parts) != 2 || m < 0 || parts < 0) return 2;
            printf("fit %d\n", sfa::query_blocks_fit(m, parts) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
