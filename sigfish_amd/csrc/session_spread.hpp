// session_spread.hpp -- the host rules of a SPREAD session (SFA_SESSION_SPREAD: the slots of one session dealt over the shards of
// a group context; pure C++, no HIP, no context; tests/c/session_spread.cpp runs them without a GPU): where a slot lives
// (spread_place and back), which entries of a call go to which shard (spread_partition: the caller's order kept inside every
// shard, local slot numbers, the caller's indices for the way back), the offset tables of a ragged payload rebuilt per shard
// (spread_offsets: ev_off, raw_off, map_off alike), and the refusals one session makes by itself -- a slot out of range, a slot
// named twice -- made here for the whole call, before anything reaches a shard: a refused call changes no shard.
// sfa_session.hip and sfa_session_targets.hip run what this returns on the shards' sub-sessions and scatter their answers (the
// visits they share: sfa_session_state.hpp).
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace sfa {

// ---- placement: global slot i lives on shard i % G with local index i / G (consecutive channels balance) ----
struct SpreadPlace {
    int32_t shard, local;
};
inline SpreadPlace spread_place(int32_t slot, int32_t g) { return SpreadPlace{slot % g, slot / g}; }
inline int32_t spread_slot(int32_t shard, int32_t local, int32_t g) { return local * g + shard; }
// slots of a session of n_slots that live on `shard` (0 for the trailing shards of a session with fewer slots than shards)
inline int32_t spread_slots_of(int32_t n_slots, int32_t shard, int32_t g) { return (n_slots - shard + g - 1) / g; }

// ---- a call's entries by shard ----
struct SpreadShardPart {
    std::vector<int32_t> local;  // local slot of the shard's entry j, in the caller's order
    std::vector<int32_t> index;  // ... and which entry of the caller's it is: results go back to out[index[j]]
    std::vector<int64_t> off;    // spread_offsets: [entries + 1], from 0, every entry as long as the caller's
    int32_t n() const { return static_cast<int32_t>(local.size()); }
};

struct SpreadPart {
    std::vector<SpreadShardPart> shard;  // [G]
    std::vector<uint8_t> seen;           // [n_slots] of the duplicate check: all zero between two calls
};

enum { kSpreadOk = 0, kSpreadRange = 1, kSpreadTwice = 2 };
struct SpreadRefusal {
    int32_t why, index, slot;  // kSpread*; the caller's entry and the slot it names
};

// The entries slot[0..n) of a call on a session of n_slots slots over g shards; slot == nullptr: every slot in order (n is
// n_slots then).  once: a slot may be named once only (the extend calls).  Everything is checked before anything is produced:
// on a refusal every shard's part is empty.  The vectors keep their capacity from call to call.
inline SpreadRefusal spread_partition(const int32_t *slot, int32_t n, int32_t n_slots, int32_t g, bool once, SpreadPart *p) {
    p->shard.resize(static_cast<size_t>(g));
    for (SpreadShardPart &s : p->shard) s.local.clear(), s.index.clear(), s.off.clear();
    SpreadRefusal bad{kSpreadOk, -1, -1};
    if (slot) {
        p->seen.resize(static_cast<size_t>(n_slots), 0);
        int32_t i = 0;
        for (; i < n && !bad.why; ++i) {
            if (slot[i] < 0 || slot[i] >= n_slots)
                bad = SpreadRefusal{kSpreadRange, i, slot[i]};
            else if (once && p->seen[slot[i]])
                bad = SpreadRefusal{kSpreadTwice, i, slot[i]};
            else if (once)
                p->seen[slot[i]] = 1;
        }
        if (once)  // (every entry in front of a refused one set its mark; the refused one set none)
            for (int32_t k = 0; k < (bad.why ? bad.index : i); ++k) p->seen[slot[k]] = 0;
        if (bad.why) return bad;
    }
    for (int32_t i = 0; i < n; ++i) {
        const SpreadPlace at = spread_place(slot ? slot[i] : i, g);
        p->shard[at.shard].local.push_back(at.local);
        p->shard[at.shard].index.push_back(i);
    }
    return bad;
}

// The offset table of every shard for a ragged payload whose entry i is [off[i], off[i + 1]) in the caller's: the shard's entries
// back to back from 0, each with its own length (an empty chunk stays an empty chunk, a length that is negative stays negative
// for the shard's own check to refuse)
inline void spread_offsets(const int64_t *off, SpreadPart *p) {
    for (SpreadShardPart &s : p->shard) {
        s.off.assign(s.index.size() + 1, 0);
        for (size_t j = 0; j < s.index.size(); ++j) s.off[j + 1] = s.off[j] + (off[s.index[j] + 1] - off[s.index[j]]);
    }
}

// the shard's chunks of src (entry i at off[i]) packed back to back into dst, which holds s.off.back() elements
template <class T>
void spread_pack(const SpreadShardPart &s, const T *src, const int64_t *off, T *dst) {
    for (size_t j = 0; j < s.index.size(); ++j) {
        const int64_t len = s.off[j + 1] - s.off[j];
        if (len > 0) memcpy(dst + s.off[j], src + off[s.index[j]], sizeof(T) * static_cast<size_t>(len));
    }
}

// per-entry values (`per` of them per entry) of the caller's into the shard's order, and a shard's answers back
template <class T>
void spread_gather(const SpreadShardPart &s, const T *from, T *to, int32_t per = 1) {
    for (size_t j = 0; j < s.index.size(); ++j)
        for (int32_t k = 0; k < per; ++k) to[j * per + k] = from[static_cast<size_t>(s.index[j]) * per + k];
}
template <class T>
void spread_scatter(const SpreadShardPart &s, const T *from, T *to, int32_t per = 1) {
    for (size_t j = 0; j < s.index.size(); ++j)
        for (int32_t k = 0; k < per; ++k) to[static_cast<size_t>(s.index[j]) * per + k] = from[j * per + k];
}

}  // namespace sfa
