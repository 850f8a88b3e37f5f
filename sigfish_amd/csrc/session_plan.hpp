// session_plan.hpp -- the host rules of a session call (pure C++, no HIP; tests/c/session_plan.cpp runs them without a GPU):
// which waves a call's chunks become (plan_session_call: the launch split at kMaxQuery events and the grouping of every launch),
// and which points of the automatic query start a slot passes when its count of samples grows (auto_points).  sfa_session.hip
// stages what they return; sdtw_session.hpp takes the class table from here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "sfa_plan.hpp"

namespace sfa {

constexpr int kSessionMaxClasses = 12;  // (first chunk or not) x the six base shapes

struct SessionClass {
    int32_t R, lanes;     // kClassShapes[...]
    int32_t first;        // 1: first chunks (constant boundary), 0: below a carried row
    int32_t group_base;   // first group (a group is one wave's worth of slots: 64 / lanes of them)
    int32_t n_groups;
    int32_t task_base;    // first task; the class has n_groups * n_jobs of them, job-major
};

// Where a slot's chunk lies in the device-resident event buffer of a call
struct Chunk {
    int64_t off, len;
};

// A piece of a slot's chunk inside one launch, and where the planner put it
struct Piece {
    int32_t call, slot, len, total, first, cls;
    int64_t off;
};

// One launch: the staging words of its tables, in the order of SessionArgs.  Entries (pieces) stand in group order
struct Launch {
    std::vector<int64_t> k_off;
    std::vector<int32_t> w_entry, g_qlen, k_call, k_slot, k_len, k_total;
    SessionClass cls[kSessionMaxClasses];
    int32_t n_cls = 0, n_tasks = 0;
};

// groups of one launch: pieces sorted by (first chunk or not, class, length modulo R, length descending), 64 / lanes of them
// per wave as long as kind, class and length modulo R agree (MixedQuad's rule: every last row in the same lane and register)
inline void plan_launch(std::vector<Piece> &pieces, int32_t n_jobs, Launch *l) {
    for (Piece &p : pieces) p.cls = class_for(p.len);
    std::sort(pieces.begin(), pieces.end(), [](const Piece &a, const Piece &b) {
        if (a.first != b.first) return a.first > b.first;
        if (a.cls != b.cls) return a.cls < b.cls;
        const int R = kClassShapes[a.cls].R;
        if (a.len % R != b.len % R) return a.len % R < b.len % R;
        if (a.len != b.len) return a.len > b.len;
        return a.call < b.call;
    });
    l->k_off.reserve(pieces.size());
    for (auto *v : {&l->k_call, &l->k_slot, &l->k_len, &l->k_total}) v->reserve(pieces.size());
    for (const Piece &p : pieces) {
        l->k_off.push_back(p.off);
        l->k_call.push_back(p.call);
        l->k_slot.push_back(p.slot);
        l->k_len.push_back(p.len);
        l->k_total.push_back(p.total);
    }
    l->n_cls = 0;
    int32_t n_groups = 0;
    for (size_t i = 0; i < pieces.size();) {
        const Piece &p = pieces[i];
        const ClassShape sh = kClassShapes[p.cls];
        if (l->n_cls == 0 || l->cls[l->n_cls - 1].first != p.first || l->cls[l->n_cls - 1].R != sh.R || l->cls[l->n_cls - 1].lanes != sh.lanes) {
            SessionClass &c = l->cls[l->n_cls++];
            c.R = sh.R;
            c.lanes = sh.lanes;
            c.first = p.first;
            c.group_base = n_groups;
            c.n_groups = 0;
            c.task_base = n_groups * n_jobs;
        }
        const int ns = 64 / sh.lanes;
        int32_t w[4] = {-1, -1, -1, -1};
        int m = 0;
        while (m < ns && i < pieces.size() && pieces[i].first == p.first && pieces[i].cls == p.cls && pieces[i].len % sh.R == p.len % sh.R) {
            w[m++] = static_cast<int32_t>(i++);
        }
        l->w_entry.insert(l->w_entry.end(), w, w + 4);
        l->g_qlen.push_back(p.len);  // (descending inside the run: the first is the longest)
        l->cls[l->n_cls - 1].n_groups++;
        ++n_groups;
    }
    l->n_tasks = n_groups * n_jobs;
}

// The launches of one call: chunk i, chunks[i], goes below the row of slot[i]; held / poison are the session's per-slot arrays
// (events a slot holds before the call; a poisoned slot is not swept).  Launch p holds events [p * kMaxQuery, (p + 1) * kMaxQuery)
// of every chunk that is that long.  call_slot[i]: slot[i] when the call sweeps it, else -1; new_events: events swept.
inline void plan_session_call(const Chunk *chunks, const int32_t *slot, const int64_t *held, const uint8_t *poison, int32_t n, int32_t n_jobs,
                              std::vector<Launch> *launches, std::vector<int32_t> *call_slot, int64_t *new_events) {
    launches->clear();
    call_slot->assign(n, -1);
    *new_events = 0;
    for (int32_t p = 0;; ++p) {
        std::vector<Piece> pieces;
        for (int32_t i = 0; i < n; ++i) {
            const int64_t l = chunks[i].len, done = static_cast<int64_t>(p) * kMaxQuery;
            if (l <= done || poison[slot[i]]) continue;
            Piece k;
            k.call = i;
            k.slot = slot[i];
            k.len = static_cast<int32_t>(std::min<int64_t>(kMaxQuery, l - done));
            k.total = static_cast<int32_t>(held[slot[i]] + done + k.len);
            k.first = (held[slot[i]] + done == 0) ? 1 : 0;
            k.off = chunks[i].off + done;
            k.cls = 0;
            pieces.push_back(k);
            if (p == 0) (*call_slot)[i] = slot[i];
            *new_events += k.len;
        }
        if (pieces.empty()) break;
        launches->emplace_back();
        plan_launch(pieces, n_jobs, &launches->back());
    }
}

// ---- automatic query start: the points a call carries a slot past (each slot's count of samples decides, not the calls) ----

struct AutoPoints {
    int32_t n0, n_periodic;  // periodic points n0, n0 + every, ... (EvAutoEntry)
    int32_t n_final;         // the final point, -1: the call brings none.  A periodic point equal to it is taken once, as the final point
    int32_t k_after;         // periodic points N_k = k * every the slot has passed after the call
    bool final_now;          // the call brings the final point: the end of the read, or the cap, whichever comes first
    bool pending;            // the call has a point to evaluate for this slot
};

// The slot's count of samples goes from `have` to `after`; ended_now: this call brings its end of read; k_done: periodic points it
// has passed already; settled: frozen, or final point already taken -- later points are not evaluated and k_done stands.
inline AutoPoints auto_points(int64_t have, int64_t after, bool ended_now, int32_t every, int32_t max_samples, int32_t k_done, bool settled) {
    AutoPoints p{0, 0, -1, k_done, false, false};
    if (settled) return p;
    const int64_t M = max_samples;
    p.k_after = every > 0 ? static_cast<int32_t>(std::min(after, M) / every) : 0;
    p.final_now = ended_now || (after >= M && have < M);
    p.n0 = (k_done + 1) * every;
    p.n_periodic = p.k_after - k_done;
    p.n_final = p.final_now ? static_cast<int32_t>(std::min(after, M)) : -1;
    p.pending = p.n_periodic > 0 || p.final_now;
    return p;
}

}  // namespace sfa
