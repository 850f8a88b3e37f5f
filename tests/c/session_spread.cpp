// session_spread.cpp -- the host rules of a spread session as the library ships them (sigfish_amd/csrc/session_spread.hpp), run
// without a GPU.  Built from that header alone; tests/test_session_spread_cpu.py builds it plain and under ASan + UBSan.
// No arguments: the checks below for G = 1, 2, 3 and 8, "ok <checks>" on success, the first failure and exit status 1 otherwise.
// With requests on stdin it answers them (the Python file compares the answers with its own restatement):
//   part G n_slots once n  slot...  off[0..n]   ->  refused <why> <index> <slot>
//                                                or  shard r <entries> | local... | index... | off...   (one line per shard)
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "session_spread.hpp"

namespace {

long g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            printf("FAILED %s:%d: %s (G %d)\n", __FILE__, __LINE__, #cond, g_G); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)
int g_G = 0;

// placement and its inverse for every slot, and the per-shard counts
void check_placement(int32_t G, int32_t n_slots) {
    std::vector<int32_t> count(G, 0);
    for (int32_t i = 0; i < n_slots; ++i) {
        const sfa::SpreadPlace at = sfa::spread_place(i, G);
        CHECK(at.shard == i % G && at.local == i / G);
        CHECK(at.shard >= 0 && at.shard < G);
        CHECK(at.local >= 0 && at.local < sfa::spread_slots_of(n_slots, at.shard, G));
        CHECK(sfa::spread_slot(at.shard, at.local, G) == i);
        ++count[at.shard];
    }
    int32_t sum = 0;
    for (int32_t r = 0; r < G; ++r) {
        CHECK(sfa::spread_slots_of(n_slots, r, G) == count[r]);
        CHECK(r == 0 || count[r] <= count[r - 1]);          // consecutive slots balance: the counts differ by one at the most
        CHECK(count[0] - count[r] <= 1);
        for (int32_t l = 0; l < count[r]; ++l) CHECK(sfa::spread_slot(r, l, G) < n_slots);
        sum += count[r];
    }
    CHECK(sum == n_slots);
}

// a call: partition, the offset tables, pack and the way back
void check_call(int32_t G, int32_t n_slots, const std::vector<int32_t> &slot, bool every_slot, sfa::SpreadPart *part) {
    const int32_t n = every_slot ? n_slots : static_cast<int32_t>(slot.size());
    const sfa::SpreadRefusal bad = sfa::spread_partition(every_slot ? nullptr : slot.data(), n, n_slots, G, true, part);
    CHECK(bad.why == sfa::kSpreadOk);
    CHECK(static_cast<int32_t>(part->shard.size()) == G);
    // chunks of 0 .. 4 values, entry i's values are 1000 * i + j: an empty chunk in the middle, and the last chunk is not empty
    std::vector<int64_t> off(n + 1, 0);
    for (int32_t i = 0; i < n; ++i) off[i + 1] = off[i] + (i == n - 1 ? 3 : (i * 7 + 3) % 5);
    std::vector<int32_t> payload(static_cast<size_t>(off[n]) + 1);
    for (int32_t i = 0; i < n; ++i)
        for (int64_t j = off[i]; j < off[i + 1]; ++j) payload[j] = 1000 * i + static_cast<int32_t>(j - off[i]);
    sfa::spread_offsets(off.data(), part);
    std::vector<int32_t> seen(n, 0), back(n, -1), answers;
    int64_t total = 0;
    for (int32_t r = 0; r < G; ++r) {
        const sfa::SpreadShardPart &p = part->shard[r];
        CHECK(p.local.size() == p.index.size() && p.off.size() == p.index.size() + 1 && p.off[0] == 0);
        std::vector<int32_t> packed(static_cast<size_t>(p.off.back()) + 1, -7);
        sfa::spread_pack(p, payload.data(), off.data(), packed.data());
        CHECK(packed[p.off.back()] == -7);  // (nothing written behind the last chunk)
        answers.assign(p.index.size(), 0);
        for (int32_t j = 0; j < p.n(); ++j) {
            const int32_t i = p.index[j], sl = every_slot ? i : slot[i];
            CHECK(j == 0 || p.index[j - 1] < i);  // the caller's order inside the shard
            CHECK(sl % G == r && sl / G == p.local[j]);
            CHECK(p.local[j] < sfa::spread_slots_of(n_slots, r, G));
            CHECK(p.off[j + 1] - p.off[j] == off[i + 1] - off[i]);  // every chunk as long as the caller's, empty ones included
            for (int64_t k = 0; k < p.off[j + 1] - p.off[j]; ++k) CHECK(packed[p.off[j] + k] == 1000 * i + k);
            ++seen[i];
            answers[j] = 10 * sl + 1;
        }
        sfa::spread_scatter(p, answers.data(), back.data());
        total += p.off.back();
    }
    CHECK(total == off[n]);
    for (int32_t i = 0; i < n; ++i) {
        CHECK(seen[i] == 1);  // every entry on exactly one shard
        CHECK(back[i] == 10 * (every_slot ? i : slot[i]) + 1);
    }
    // gather is scatter's inverse, `per` values per entry
    std::vector<double> three(3 * static_cast<size_t>(n)), there, again(3 * static_cast<size_t>(n), -1.0);
    std::iota(three.begin(), three.end(), 0.5);
    for (int32_t r = 0; r < G; ++r) {
        there.assign(3 * part->shard[r].index.size(), 0.0);
        sfa::spread_gather(part->shard[r], three.data(), there.data(), 3);
        sfa::spread_scatter(part->shard[r], there.data(), again.data(), 3);
    }
    CHECK(again == three);
}

void check_refusals(int32_t G, int32_t n_slots, sfa::SpreadPart *part) {
    auto refused = [&](std::vector<int32_t> slot, bool once, int32_t why, int32_t index) {
        // (a call that went through before: a refusal must leave no part of it, and none of the refused call)
        CHECK(sfa::spread_partition(nullptr, n_slots, n_slots, G, true, part).why == sfa::kSpreadOk);
        const sfa::SpreadRefusal bad = sfa::spread_partition(slot.data(), static_cast<int32_t>(slot.size()), n_slots, G, once, part);
        CHECK(bad.why == why && bad.index == index && bad.slot == slot[index]);
        for (const sfa::SpreadShardPart &p : part->shard) CHECK(p.local.empty() && p.index.empty() && p.off.empty());  // before any partition is produced
        for (uint8_t m : part->seen) CHECK(m == 0);  // and the next call starts clean
    };
    refused({n_slots}, true, sfa::kSpreadRange, 0);
    refused({0, n_slots + 5}, false, sfa::kSpreadRange, 1);
    refused({-1}, true, sfa::kSpreadRange, 0);
    refused({0, -3}, false, sfa::kSpreadRange, 1);
    refused({0, 0}, true, sfa::kSpreadTwice, 1);
    if (n_slots >= 3) {
        refused({0, 2, 0}, true, sfa::kSpreadTwice, 2);
        refused({2, 1, 1, n_slots}, true, sfa::kSpreadTwice, 2);  // the first refusal in the caller's order
        refused({2, n_slots, 1, 1}, true, sfa::kSpreadRange, 1);
    }
    // calls that may name a slot twice (lengths, candidates, maps: one slot any number of times)
    std::vector<int32_t> twice{0, 0, n_slots - 1, 0};
    CHECK(sfa::spread_partition(twice.data(), 4, n_slots, G, false, part).why == sfa::kSpreadOk);
    size_t entries = 0;
    for (const sfa::SpreadShardPart &p : part->shard) entries += p.index.size();
    CHECK(entries == 4);
}

int self_check() {
    for (int32_t G : {1, 2, 3, 8}) {
        g_G = G;
        sfa::SpreadPart part;  // one for all calls, as a session keeps it
        for (int32_t n_slots : {1, G - 1, G, G + 1, 37}) {
            if (n_slots < 1) continue;
            check_placement(G, n_slots);
            std::vector<int32_t> all(n_slots), desc(n_slots), one_shard;
            std::iota(all.begin(), all.end(), 0);
            for (int32_t i = 0; i < n_slots; ++i) desc[i] = n_slots - 1 - i;
            const int32_t r = (G - 1) < n_slots ? G - 1 : 0;  // the last shard that holds a slot
            for (int32_t sl = r; sl < n_slots; sl += G) one_shard.push_back(sl);
            check_call(G, n_slots, {}, true, &part);             // every slot, no list
            check_call(G, n_slots, all, false, &part);           // every slot, named
            check_call(G, n_slots, {n_slots - 1}, false, &part); // one slot
            check_call(G, n_slots, one_shard, false, &part);     // only slots of one shard
            check_call(G, n_slots, desc, false, &part);          // descending order
            const sfa::SpreadRefusal none = sfa::spread_partition(all.data(), 0, n_slots, G, true, &part);  // no slot at all
            CHECK(none.why == sfa::kSpreadOk);
            const int64_t zero = 0;
            sfa::spread_offsets(&zero, &part);
            for (const sfa::SpreadShardPart &p : part.shard) CHECK(p.n() == 0 && p.off.size() == 1 && p.off[0] == 0);
            for (int32_t q = 0; q < G; ++q)  // one shard only: the others have no entries
                if (q != r) {
                    CHECK(sfa::spread_partition(one_shard.data(), static_cast<int32_t>(one_shard.size()), n_slots, G, true, &part).why == sfa::kSpreadOk);
                    CHECK(part.shard[q].n() == 0 && part.shard[r].n() == static_cast<int32_t>(one_shard.size()));
                }
            check_refusals(G, n_slots, &part);
        }
    }
    printf("ok %ld\n", g_checks);
    return 0;
}

int answer_requests() {
    char tag[16];
    sfa::SpreadPart part;
    while (scanf("%15s", tag) == 1) {
        int G, n_slots, once, n;
        if (scanf("%d %d %d %d", &G, &n_slots, &once, &n) != 4) return 2;
        std::vector<int32_t> slot(n);
        std::vector<int64_t> off(n + 1);
        for (int i = 0; i < n; ++i)
            if (scanf("%d", &slot[i]) != 1) return 2;
        for (int i = 0; i <= n; ++i) {
            long long v;
            if (scanf("%lld", &v) != 1) return 2;
            off[i] = v;
        }
        const sfa::SpreadRefusal bad = sfa::spread_partition(slot.data(), n, n_slots, G, once != 0, &part);
        if (bad.why) {
            printf("refused %d %d %d\n", bad.why, bad.index, bad.slot);
            continue;
        }
        sfa::spread_offsets(off.data(), &part);
        for (int r = 0; r < G; ++r) {
            const sfa::SpreadShardPart &p = part.shard[r];
            printf("shard %d %d |", r, p.n());
            for (int32_t v : p.local) printf(" %d", v);
            printf(" |");
            for (int32_t v : p.index) printf(" %d", v);
            printf(" |");
            for (int64_t v : p.off) printf(" %lld", static_cast<long long>(v));
            printf("\n");
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char **) { return argc > 1 ? answer_requests() : self_check(); }
