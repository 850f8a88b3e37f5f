// reach_group_rules.hpp -- the host rules of a session's reach groups (sfa_session_target_groups_reach,
// sfa_session_group_reach_tables; pure C++, no HIP, no context; tests/c/reach_group_rules.cpp runs them without a GPU).  Admission,
// the anchor of a target and of a column, the entries of a depth track and the sweep over cuts are reach_rules.hpp's; the label
// table, its padding and the refusals for group ids are group_rules.hpp's; place_col and the depth track are row_rules.hpp's and
// coverage_rules.hpp's; nothing of them is restated here.
// A reach group target is a reach target with a group id: WHICH named target will the read run into?
//   * admission: reach_admits on the target's reach fields (reach_group_reach_of).
//   * the anchor of a column: reach_tables' anchor of the list with the groups dropped -- groups do not enter it.
//   * the label of a column: the lowest group id among the admitting targets whose OWN anchor (reach_anchor_of) equals the
//     column's anchor -- the target the read reaches first, ties to the lowest id; n_groups, the background, when nobody admits
//     the column.  So: with every lead 0 and every strand 0 the table is group_labels' bit for bit; a label is a group exactly
//     where reach_tables sets the mask bit; inside a body another group's lead-in never takes the label (the body's anchor x beats
//     any begin > x).
//   * what a list is refused for (reach_group_list_error): group_list_error's refusal of n_groups, everything reach_list_error
//     refuses (its words), group_list_error's refusal of a group id.
//   * the model (reach_group_tables): a loop over columns and targets, as the rule reads.
//   * the prepared form the device bisects (reach_group_prepare): per job, rising disjoint runs {lo, hi, a, step, label}; the
//     entry of column j is a + step * j as in a ReachRun.  It is reach_prepare's sweep over cuts with the covering bodies kept
//     in a heap by group id (the lowest group among the bodies over a piece) and the open lead-ins in a heap by (b, group) (the
//     nearest body in front, and the lowest group among the lead-ins that lead to it).  Both heaps drop what has ended when it
//     comes to the top, so the sweep is O(n log n) in the targets.  A run ends where the anchor rule or the label changes.
//   * the live label under a group cap (reach_group_live_label): the base label while the depth of the ANCHOR's entry lies below
//     the cap (kReachBelowTrack: depth 0, as in reach_live), the background from then on; a background column reads no depth.
//   * the depth records on a reach label table (reach_group_counts): the '+' jobs' BODY columns only, by base label -- a body
//     column is one whose anchor entry is its own track entry.  A lead-in column is part of no record: it reports a coordinate
//     that belongs to no target.  A group that has only '-' targets therefore has an empty record.
// sdtw_session_reachgroup.hpp builds the two tables from the runs and derives the live labels from labels, anchors and depth.
#pragma once

#include <queue>

#include "group_cover_rules.hpp"
#include "reach_rules.hpp"

namespace sfa {

static_assert(sizeof(sfa_reach_group_target_t) == 24, "sfa_reach_group_target_t is five int32 and four bytes: the bindings mirror it");

// bytes the feature takes on a session: the label table's 2 bytes and the anchor's 4 per column
inline size_t reach_group_bytes(const int64_t total_cols) { return (2 + 4) * static_cast<size_t>(total_cols); }

// the reach fields of a target
inline sfa_reach_target_t reach_group_reach_of(const sfa_reach_group_target_t &t) {
    sfa_reach_target_t r{};
    r.contig = t.contig, r.begin = t.begin, r.end = t.end, r.lead = t.lead, r.strand = t.strand;
    r.pad[0] = t.pad[0], r.pad[1] = t.pad[1], r.pad[2] = t.pad[2];
    return r;
}
// the list with the groups dropped
inline std::vector<sfa_reach_target_t> reach_group_reach_list(const sfa_reach_group_target_t *t, const int32_t n) {
    std::vector<sfa_reach_target_t> r(static_cast<size_t>(n));
    for (int32_t k = 0; k < n; ++k) r[static_cast<size_t>(k)] = reach_group_reach_of(t[k]);
    return r;
}

// nullptr, or why the list is refused (the text in msg)
inline const char *reach_group_list_error(const sfa_reach_group_target_t *t, int32_t n, int32_t n_groups, const TargetModel &m, char *msg, size_t cap) {
    if (group_list_error(nullptr, 0, n_groups, m, msg, cap)) return msg;         // n_groups
    if (n > kReachTargetsMax) return reach_list_error(nullptr, n, m, msg, cap);  // (the count comes first: the list is not read)
    const std::vector<sfa_reach_target_t> reach = reach_group_reach_list(t, n);
    if (reach_list_error(reach.data(), n, m, msg, cap)) return msg;
    std::vector<sfa_group_target_t> plain(static_cast<size_t>(n));
    for (int32_t k = 0; k < n; ++k) plain[static_cast<size_t>(k)] = sfa_group_target_t{t[k].contig, t[k].begin, t[k].end, t[k].group};
    return group_list_error(plain.data(), n, n_groups, m, msg, cap);  // (the intervals have passed: only a group id is left to refuse)
}

// The model: labels (4 * group_label_words entries, the padding holds the background) and anchor COORDINATES ([total_cols], -1:
// none) of a checked list; returns the columns that belong to a group
inline int64_t reach_group_tables(const sfa_reach_group_target_t *t, int32_t n, int32_t n_groups, const TargetModel &m, std::vector<uint16_t> *label,
                                  std::vector<int32_t> *anchor) {
    const uint16_t bg = static_cast<uint16_t>(n_groups);
    label->assign(4 * group_label_words(m.total_cols), bg);
    anchor->assign(static_cast<size_t>(m.total_cols), kReachNone);
    const std::vector<sfa_reach_target_t> reach = reach_group_reach_list(t, n);
    int64_t in = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        const int strand = m.job_strand[j];
        for (int32_t col = 0; col < m.job_len[j]; ++col) {
            const int32_t x = place_col(strand, col, rl, off);
            bool any = false;
            int32_t best = kReachNone;
            for (int32_t k = 0; k < n; ++k) {  // the column's anchor: groups do not enter it
                if (!reach_admits(reach[static_cast<size_t>(k)], contig, strand, x)) continue;
                const int32_t a = reach_anchor_of(reach[static_cast<size_t>(k)], strand, x);
                best = !any ? a : (strand == '+' ? std::min(best, a) : std::max(best, a));
                any = true;
            }
            if (!any) continue;
            int32_t g = n_groups;
            for (int32_t k = 0; k < n; ++k)  // the lowest group among the targets the read reaches first
                if (reach_admits(reach[static_cast<size_t>(k)], contig, strand, x) && reach_anchor_of(reach[static_cast<size_t>(k)], strand, x) == best) g = std::min(g, t[k].group);
            const size_t c = static_cast<size_t>(m.col_off[j] + col);
            (*label)[c] = static_cast<uint16_t>(g);
            (*anchor)[c] = best;
            ++in;
        }
    }
    return in;
}

// ---- the prepared form ----
struct ReachGroupRun {
    int32_t lo, hi;   // columns [lo, hi) of the job
    int32_t a, step;  // entry of column j: a + step * j; step 0 and a = kReachBelowTrack: no entry
    int32_t label;    // the group of every column of the run
};
struct ReachGroupPrepared {
    std::vector<int32_t> run_off;  // [n_jobs + 1]: job j's runs are runs[run_off[j] .. run_off[j + 1])
    std::vector<ReachGroupRun> runs;
};

// the run of `runs[0 .. n)` (rising, disjoint) that holds column j, or -1
SFA_ROW_HD int32_t reach_group_find_run(const ReachGroupRun *runs, const int32_t n, const int32_t j) {
    int32_t lo = 0, hi = n;  // the first run whose lo lies beyond j
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (runs[mid].lo <= j)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo > 0 && j < runs[lo - 1].hi) ? lo - 1 : -1;
}
SFA_ROW_HD int32_t reach_group_run_entry(const ReachGroupRun &r, const int32_t j) { return r.a + r.step * j; }

inline void reach_group_prepare(const sfa_reach_group_target_t *t, int32_t n, const TargetModel &m, ReachGroupPrepared *p) {
    p->run_off.assign(static_cast<size_t>(m.n_jobs) + 1, 0);
    p->runs.clear();
    // the targets of every contig, in list order
    std::vector<int32_t> first(static_cast<size_t>(m.num_ref) + 1, 0), order(static_cast<size_t>(n));
    for (int32_t k = 0; k < n; ++k) ++first[static_cast<size_t>(t[k].contig) + 1];
    for (int32_t c = 0; c < m.num_ref; ++c) first[static_cast<size_t>(c) + 1] += first[static_cast<size_t>(c)];
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for (int32_t k = 0; k < n; ++k) order[static_cast<size_t>(at[static_cast<size_t>(t[k].contig)]++)] = k;
    }
    // reach_prepare's rising coordinate u (u = x on '+', u = -x on '-', column = u + shift): a target is a body [B, E) with a
    // lead-in [B - lead, B) whose columns lead to B
    struct Piece {
        int64_t lo, hi, b;  // [lo, hi) in u, clipped to the job's; b: the body's first u (a lead-in's value)
        int32_t group;
    };
    std::vector<Piece> body, lead;
    std::vector<int64_t> cut;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        const int strand = m.job_strand[j];
        const bool plus = strand == '+';
        const int64_t shift = plus ? -static_cast<int64_t>(off) : static_cast<int64_t>(rl) + off;  // column = u + shift
        const int64_t ulo = -shift, uhi = m.job_len[j] - shift;                                    // the job's columns in u
        body.clear(), lead.clear(), cut.clear();
        for (int32_t q = first[static_cast<size_t>(contig)]; q < first[static_cast<size_t>(contig) + 1]; ++q) {
            const sfa_reach_group_target_t &x = t[order[static_cast<size_t>(q)]];
            if (x.strand != 0 && x.strand != strand) continue;
            const int64_t b = plus ? static_cast<int64_t>(x.begin) : -(static_cast<int64_t>(x.end) - 1);
            const int64_t e = plus ? static_cast<int64_t>(x.end) : -static_cast<int64_t>(x.begin) + 1;
            const Piece bd = {std::max(b, ulo), std::min(e, uhi), b, x.group}, ld = {std::max(b - x.lead, ulo), std::min(b, uhi), b, x.group};
            if (bd.lo < bd.hi) body.push_back(bd), cut.push_back(bd.lo), cut.push_back(bd.hi);
            if (ld.lo < ld.hi) lead.push_back(ld), cut.push_back(ld.lo), cut.push_back(ld.hi);
        }
        std::sort(cut.begin(), cut.end());
        cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
        const auto by_lo = [](const Piece &x, const Piece &y) { return x.lo < y.lo; };
        std::sort(body.begin(), body.end(), by_lo);
        std::sort(lead.begin(), lead.end(), by_lo);
        // between two cuts the rule is one.  Over a body the anchor is the column's own coordinate, and the targets whose own
        // anchor that is are the bodies over the piece: the lowest group of them (a heap by group; a body that has ended goes
        // when it comes to the top).  Else the nearest body in front among the lead-ins over the piece, and the lowest group
        // among those that lead to it (a heap by (b, group)).
        const auto higher_group = [](const Piece &x, const Piece &y) { return x.group > y.group; };
        const auto later = [](const Piece &x, const Piece &y) { return x.b != y.b ? x.b > y.b : x.group > y.group; };
        std::priority_queue<Piece, std::vector<Piece>, decltype(higher_group)> over(higher_group);
        std::priority_queue<Piece, std::vector<Piece>, decltype(later)> open(later);
        size_t bi = 0, li = 0;
        const size_t run0 = p->runs.size();
        for (size_t i = 0; i + 1 < cut.size(); ++i) {
            const int64_t lo = cut[i], hi = cut[i + 1];
            while (bi < body.size() && body[bi].lo <= lo) over.push(body[bi++]);
            while (li < lead.size() && lead[li].lo <= lo) open.push(lead[li++]);
            while (!over.empty() && over.top().hi <= lo) over.pop();
            while (!open.empty() && open.top().b <= lo) open.pop();
            ReachGroupRun r = {static_cast<int32_t>(lo + shift), static_cast<int32_t>(hi + shift), 0, 0, 0};
            if (!over.empty()) {
                r.a = plus ? 0 : rl, r.step = plus ? 1 : -1;
                r.label = over.top().group;
            } else if (!open.empty()) {
                const int64_t coord = plus ? open.top().b : -open.top().b;  // (a target's begin on '+', its end - 1 on '-')
                r.a = reach_entry_of(static_cast<int32_t>(coord), off);
                r.label = open.top().group;
            } else {
                continue;
            }
            if (p->runs.size() > run0 && p->runs.back().hi == r.lo && p->runs.back().a == r.a && p->runs.back().step == r.step && p->runs.back().label == r.label)
                p->runs.back().hi = r.hi;
            else
                p->runs.push_back(r);
        }
        p->run_off[static_cast<size_t>(j) + 1] = static_cast<int32_t>(p->runs.size());
    }
}

// The tables the runs give when every column bisects them, as the build kernel does: labels (4 * group_label_words entries, the
// padding holds the background) and anchor ENTRIES ([total_cols]: an index into the contig's track, kReachNone,
// kReachBelowTrack); returns the columns that belong to a group
inline int64_t reach_group_tables_from_runs(const ReachGroupPrepared &p, int32_t n_groups, const TargetModel &m, std::vector<uint16_t> *label, std::vector<int32_t> *entry) {
    label->assign(4 * group_label_words(m.total_cols), static_cast<uint16_t>(n_groups));
    entry->assign(static_cast<size_t>(m.total_cols), kReachNone);
    int64_t in = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const ReachGroupRun *runs = p.runs.data() + p.run_off[static_cast<size_t>(j)];
        const int32_t n_runs = p.run_off[static_cast<size_t>(j) + 1] - p.run_off[static_cast<size_t>(j)];
        for (int32_t col = 0; col < m.job_len[j]; ++col) {
            const int32_t r = reach_group_find_run(runs, n_runs, col);
            if (r < 0) continue;
            const size_t c = static_cast<size_t>(m.col_off[j] + col);
            (*label)[c] = static_cast<uint16_t>(runs[r].label);
            (*entry)[c] = reach_group_run_entry(runs[r], col);
            ++in;
        }
    }
    return in;
}

// ---- the live label under a group cap: the base label while the depth of the ANCHOR's entry lies below the cap ----
SFA_ROW_HD uint16_t reach_group_live_label(const uint16_t base, const uint32_t *track, const int32_t entry, const int32_t track_len, const uint32_t cap, const uint16_t bg) {
    if (base == bg) return bg;                           // (a background column reads no depth)
    if (entry < 0 || entry >= track_len) return base;    // (kReachBelowTrack: depth 0; an entry beyond the track never leaves reach_group_prepare)
    return track[entry] < cap ? base : bg;
}

// does column j of a job count in the depth records of a reach label table?  ('+' jobs, body columns: the anchor is the column's own entry)
SFA_ROW_HD bool reach_group_counts(const int strand, const int32_t entry, const int32_t j, const int32_t rl, const int32_t off) {
    return group_cover_counts(strand) && entry == coverage_entry(strand, j, rl, off);
}

// The live table of a base table and its entries under depth and cap into `live` (the padding holds the background) and the
// lowest column of every live label into `first` (n_groups + 1 entries, kNoColumn: none); returns the columns whose live label is a group
inline int64_t reach_group_live_labels(const std::vector<uint16_t> &base, const std::vector<int32_t> &entry, const uint32_t *depth, const int64_t *cov_off, const uint32_t cap,
                                       const int32_t n_groups, const TargetModel &m, std::vector<uint16_t> *live, std::vector<int32_t> *first) {
    const uint16_t bg = static_cast<uint16_t>(n_groups);
    live->assign(4 * group_label_words(m.total_cols), bg);
    first->assign(static_cast<size_t>(n_groups) + 1, kNoColumn);
    int64_t in = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j];
        for (int32_t k = 0; k < m.job_len[j]; ++k) {
            const size_t g = static_cast<size_t>(m.col_off[j] + k);
            const uint16_t l = reach_group_live_label(base[g], depth + cov_off[contig], entry[g], coverage_track_len(m.ref_len[contig]), cap, bg);
            (*live)[g] = l;
            if ((*first)[l] == kNoColumn) (*first)[l] = static_cast<int32_t>(g);  // (columns in rising order)
            in += l != bg;
        }
    }
    return in;
}

// The records of the n_groups + 1 entries from the base table, its entries, the depth and the cap
inline void reach_group_records(const std::vector<uint16_t> &base, const std::vector<int32_t> &entry, const uint32_t *depth, const int64_t *cov_off, const uint32_t cap,
                                const int32_t n_groups, const TargetModel &m, std::vector<sfa_group_cover_t> *rec) {
    rec->assign(static_cast<size_t>(n_groups) + 1, group_cover_none());
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        for (int32_t k = 0; k < m.job_len[j]; ++k) {
            const size_t g = static_cast<size_t>(m.col_off[j] + k);
            if (!reach_group_counts(m.job_strand[j], entry[g], k, rl, off)) continue;
            group_cover_note((*rec)[base[g]], depth[cov_off[contig] + entry[g]], cap);
        }
    }
}

}  // namespace sfa
