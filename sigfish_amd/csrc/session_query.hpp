// session_query.hpp -- which entries of a session's query call launch (sfa_session_classes, sfa_session_group_bests,
// sfa_session_open_classes; the skeleton they share is query_run of sfa_session_targets.hip).  Plain C++, no HIP: the same header
// builds into the stand-alone program tests/c/session_query.cpp.
//
// Entry i of a call names slot[i].  A slot that is poisoned or has received no events has no carried row: its entry is not
// launched and keeps the call's "none" record.  The others are launched in the caller's order: launched entry k is the caller's
// entry live[k], so its slot is slot[live[k]] and its record goes to out[live[k]] (the scatter index).  A call launches
// m x parts blocks, m the launched entries and parts the pieces of a row (class_parts): more than 2^31 - 1 of them is refused.
#pragma once
#include <cstdint>
#include <vector>

namespace sfa {

// live: the caller's indices of the entries that launch, ascending.  poison[] and len[] are the session's, by slot; every
// slot[i] is one of its slots (the caller has checked)
inline void query_live_entries(const int32_t *slot, int32_t n, const uint8_t *poison, const int64_t *len, std::vector<int32_t> *live) {
    live->clear();
    for (int32_t i = 0; i < n; ++i)
        if (!poison[slot[i]] && len[slot[i]] > 0) live->push_back(i);
}

// the slot list as it is uploaded: h_slot[k], k < live.size(), is the slot of launched entry k
inline void query_live_slots(const int32_t *slot, const std::vector<int32_t> &live, int32_t *h_slot) {
    for (size_t k = 0; k < live.size(); ++k) h_slot[k] = slot[live[k]];
}

// the way back: put(k, i, slot) for every launched entry k, i the caller's entry its record goes to and slot the slot it names
template <class F>
inline void query_scatter(const int32_t *slot, const std::vector<int32_t> &live, F put) {
    for (size_t k = 0; k < live.size(); ++k) put(static_cast<int32_t>(k), live[k], slot[live[k]]);
}

// m launched entries x parts blocks each: what one launch takes
inline bool query_blocks_fit(int32_t m, int32_t parts) { return static_cast<int64_t>(m) * parts <= INT32_MAX; }

}  // namespace sfa
