// group_rules.hpp -- the host rules of a session's target groups (sfa_session_target_groups, sfa_session_group_bests; pure C++, no
// HIP, no context; tests/c/group_rules.cpp runs them without a GPU):
//   * which group every column of a slot's row belongs to (group_labels): one uint16 per column of the concatenated column space,
//     job after job in the order of the rows' col_off -- the layout of the mask of target_rules.hpp.  A column is covered by an
//     interval under the mask's reading (place_col of row_rules.hpp: the coordinate of an alignment ENDING in it); a column
//     covered by intervals of several groups belongs to the lowest group id, a column covered by none to the background, label
//     n_groups.  An interval is a run of columns whose two ends are bisected over place_col (target_first_col): the mapping is
//     stated in row_rules.hpp only.
//   * what a list of group targets is refused for (group_list_error: target_list_error's refusals, a bad group id, a bad n_groups)
//   * the key of a column, (bits of its cost << 32) | column, whose unsigned minimum IS the tie rule of class_before (lowest cost,
//     then lowest column of the row) for the costs a carried row holds.  A carried row's cell is cn = fabsf(x - y) + m with m the minimum of
//     three cells of the same kind, +0 in a query's first row or +inf at a forced boundary (the fill's cell, sdtw_kernels.hpp,
//     which the session sweep of sdtw_session.hpp shares: "all arithmetic is the fill's"): a sum of absolute differences of finite floats, so it is
//     >= +0, possibly +inf (3e38 + 3e38), never NaN (nothing is subtracted from an infinity, no 0 * inf) and never -0 (fabsf
//     clears the sign, and a sum of two values that are not -0 is not -0 under round-to-nearest).  For such floats the unsigned
//     order of the bit patterns is the order of the values, and equal values are equal bits.  The claim does NOT hold for the
//     pad words around a row (+-3.4e38 markers) -- no pad word is ever offered -- nor for a poisoned slot (NaN events), which
//     the host does not launch.  All-ones is no column's key (its cost word would be a NaN): it says `no column met`.
//   * the head of a slot (group_head: the two smallest keys of its n_groups + 1 entries) and the decision (group_decide)
// sdtw_session_group.hpp reduces the rows under the labels with group_key and places the winners with class_place.
#pragma once

#include <string.h>

#include "target_rules.hpp"

namespace sfa {

constexpr int32_t kGroupMax = 1023;               // n_groups at most: with the background 1024 entries, 8 KB of keys in LDS
constexpr uint64_t kGroupNoKey = ~uint64_t{0};    // nothing was offered

// 8-byte words of the label table of a row of total_cols columns, and one more: the kernel reads the word behind a quad's own
inline size_t group_label_words(int64_t total_cols) { return static_cast<size_t>((total_cols + 3) / 4) + 1; }

// nullptr, or why the list is refused (the text in msg)
inline const char *group_list_error(const sfa_group_target_t *t, int32_t n, int32_t n_groups, const TargetModel &m, char *msg, size_t cap) {
    if (n_groups < 1 || n_groups > kGroupMax) {
        snprintf(msg, cap, "n_groups %d is not in 1 .. %d", n_groups, kGroupMax);
        return msg;
    }
    for (int32_t k = 0; k < n; ++k) {
        const sfa_target_t x{t[k].contig, t[k].begin, t[k].end};
        if (target_list_error(&x, 1, m, msg, cap)) {  // (its text names target 0: say which one it was)
            char inner[192];
            snprintf(inner, sizeof inner, "%s", msg + (strncmp(msg, "target 0: ", 10) == 0 ? 10 : 0));
            snprintf(msg, cap, "target %d: %s", k, inner);
            return msg;
        }
        if (t[k].group < 0 || t[k].group >= n_groups) {
            snprintf(msg, cap, "target %d: group %d out of range (n_groups is %d)", k, t[k].group, n_groups);
            return msg;
        }
    }
    return nullptr;
}

// The labels of the list (checked by group_list_error) into `label` (4 * group_label_words entries, the padding holds the
// background); returns the columns that belong to a group
inline int64_t group_labels(const sfa_group_target_t *t, int32_t n, int32_t n_groups, const TargetModel &m, std::vector<uint16_t> *label) {
    const uint16_t bg = static_cast<uint16_t>(n_groups);
    label->assign(4 * group_label_words(m.total_cols), bg);
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.job_len[j], off = m.ref_st_offset[contig];
        const int strand = m.job_strand[j];
        const bool rising = place_col(strand, 1, rl, off) > place_col(strand, 0, rl, off);
        for (int32_t k = 0; k < n; ++k) {
            if (t[k].contig != contig) continue;
            const int32_t b = t[k].begin, e = t[k].end;
            // the run of target_mask: [first x >= b, first x >= e) along a rising coordinate, [first x < e, first x < b) along a falling one
            const int32_t lo = rising ? target_first_col(strand, rl, off, [&](int x) { return x >= b; }) : target_first_col(strand, rl, off, [&](int x) { return x < e; });
            const int32_t hi = rising ? target_first_col(strand, rl, off, [&](int x) { return x >= e; }) : target_first_col(strand, rl, off, [&](int x) { return x < b; });
            const uint16_t g = static_cast<uint16_t>(t[k].group);
            for (int64_t c = m.col_off[j] + lo; c < m.col_off[j] + hi; ++c) (*label)[static_cast<size_t>(c)] = std::min((*label)[static_cast<size_t>(c)], g);  // (bg is the largest)
        }
    }
    int64_t in = 0;
    for (int64_t c = 0; c < m.total_cols; ++c) in += (*label)[static_cast<size_t>(c)] != bg;
    return in;
}

// ---- the key of a column ----
SFA_ROW_HD uint64_t group_key(const float cost, const int32_t col) {
    return (static_cast<uint64_t>(static_cast<uint32_t>(row_bits(cost))) << 32) | static_cast<uint32_t>(col);
}
SFA_ROW_HD float group_key_cost(const uint64_t key) { return key == kGroupNoKey ? INFINITY : row_float(static_cast<int32_t>(key >> 32)); }
SFA_ROW_HD int32_t group_key_col(const uint64_t key) { return key == kGroupNoKey ? kNoColumn : static_cast<int32_t>(key & 0xffffffffu); }

// One entry from its key and the place of its column
SFA_ROW_HD sfa_group_best_t group_best_of(const uint64_t key, const ClassPlace &p) {
    sfa_group_best_t b;
    b.score = group_key_cost(key);
    b.rid = p.rid;
    b.pos_end = p.pos_end;
    b.strand = p.strand;
    b.pad[0] = b.pad[1] = b.pad[2] = 0;
    return b;
}

// The two smallest keys with their entries, merged pairwise: (k1, e1) the smallest, (k2, e2) the next, of DISJOINT sets of
// entries.  Keys of entries that have a column are distinct (the column is part of the key); kGroupNoKey never wins a place.
struct GroupTop2 {
    uint64_t k1, k2;
    int32_t e1, e2;
};
SFA_ROW_HD GroupTop2 group_top2_none() { return GroupTop2{kGroupNoKey, kGroupNoKey, -1, -1}; }
SFA_ROW_HD void group_top2_offer(GroupTop2 &t, const uint64_t key, const int32_t entry) {
    if (key == kGroupNoKey) return;
    if (key < t.k1) {
        t.k2 = t.k1, t.e2 = t.e1;
        t.k1 = key, t.e1 = entry;
    } else if (key < t.k2) {
        t.k2 = key, t.e2 = entry;
    }
}
SFA_ROW_HD GroupTop2 group_top2_merge(const GroupTop2 &a, const GroupTop2 &b) {
    const bool take = b.k1 < a.k1;  // the winner's own runner-up, or the loser's best
    const GroupTop2 &w = take ? b : a, &l = take ? a : b;
    const bool second_is_losers = l.k1 < w.k2;
    return GroupTop2{w.k1, second_is_losers ? l.k1 : w.k2, w.e1, second_is_losers ? l.e1 : w.e2};
}
SFA_ROW_HD sfa_group_head_t group_head_of(const GroupTop2 &t) {
    sfa_group_head_t h;
    h.best = t.e1;
    h.second = t.e2;
    h.best_score = group_key_cost(t.k1);
    h.second_score = group_key_cost(t.k2);
    h.n_events = 0;  // (the host's: it knows the slots' lengths)
    h.valid = 1;
    return h;
}
inline sfa_group_head_t group_head(const uint64_t *keys, const int32_t n_entries) {
    GroupTop2 t = group_top2_none();
    for (int32_t e = 0; e < n_entries; ++e) group_top2_offer(t, keys[e], e);
    return group_head_of(t);
}
inline sfa_group_head_t group_head_none() { return sfa_group_head_t{-1, -1, INFINITY, INFINITY, 0, 0}; }

// ---- the decision: the best entry's index, or -1 ----
inline int32_t group_decide(const sfa_group_head_t &h, const int32_t min_events, const float margin) {
    if (!h.valid || h.best < 0 || h.n_events < min_events || !(margin >= 0.0f) || !isfinite(margin)) return -1;
    const float second = h.second < 0 ? INFINITY : h.second_score;
    return second - h.best_score >= margin * static_cast<float>(h.n_events) ? h.best : -1;  // (inf - inf is NaN: no decision)
}

}  // namespace sfa
