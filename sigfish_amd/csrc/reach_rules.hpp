// reach_rules.hpp -- the host rules of a session's reach targets (sfa_session_targets_reach, sfa_session_reach_tables; pure C++, no
// HIP, no context; tests/c/reach_rules.cpp runs them without a GPU).  The mask layout, place_col, TargetModel and the depth track
// are target_rules.hpp's, row_rules.hpp's and coverage_rules.hpp's; nothing of them is restated here.
// A plain target asks where a read's alignment ENDS now.  A read goes on from there: on '+' towards higher coordinates, on '-'
// towards lower ones.  A reach target is a target with a strand and a lead: the bases IN FRONT of it, in the read's direction,
// from which the read will run into it.
//   * the rule (reach_admits): with x = place_col of column j of job (contig c, strand s), target t admits the column when
//     t.contig == c, t.strand is 0 or s, and  t.begin - t.lead <= x < t.end  on '+',  t.begin <= x < t.end + t.lead  on '-'.  The
//     bounds are 64-bit; only the coordinates a row reports clip them.  A column is ON target when some target admits it.
//   * the anchor (reach_anchor_of): the first base of a target the read will reach -- on '+' the minimum over the admitting
//     targets of max(x, t.begin), on '-' the maximum of min(x, t.end - 1); -1 when nobody admits the column.  A depth cap reads
//     the depth of the ANCHOR, not of x: a lead-in closes when the bases it leads to are covered.  With every lead 0 and every
//     strand 0 the mask is target_mask's and the anchor is x.
//   * what a list is refused for (reach_list_error): more than 2^20 targets, everything target_list_error refuses (its messages),
//     a lead outside 0 .. 2^30, a strand other than 0, '+', '-', padding that is not zero.
//   * the model (reach_tables): a loop over columns and targets, as the rule reads.
//   * the prepared form the device bisects (reach_prepare): per job, runs of disjoint column ranges in rising order, each with its
//     anchor rule -- `entry = a + step * column`, step 0 for a lead-in (every column leads to one base), +1 / -1 inside a target's
//     body (the anchor is the column's own coordinate).  An entry is an index into the contig's depth track (coverage_rules.hpp:
//     coordinate - ref_st_offset).  On '-' a target that ends at or below ref_st_offset has an anchor no row reports and no
//     interval is counted at: its entry is kReachBelowTrack, whose depth is 0 by definition.  O(n log n) in the targets.
// sdtw_session_reach.hpp builds the mask and the anchor table from the runs and derives the live mask from mask, anchors and depth.
#pragma once

#include <string.h>

#include <queue>
#include <string>

#include "coverage_rules.hpp"

namespace sfa {

constexpr int32_t kReachLeadMax = 1 << 30;     // the largest lead
constexpr int32_t kReachTargetsMax = 1 << 20;  // targets of one list
constexpr int32_t kReachNone = -1;             // the anchor (coordinate or entry) of a column nobody admits
constexpr int32_t kReachBelowTrack = -2;       // entry of an anchor below ref_st_offset: no track entry, depth 0

static_assert(sizeof(sfa_reach_target_t) == 20, "sfa_reach_target_t is four int32 and four bytes: the bindings mirror it");

// bytes the feature adds to a session beside the mask: one anchor per column
inline size_t reach_bytes(const int64_t total_cols) { return 4 * static_cast<size_t>(total_cols); }

// nullptr, or why the list is refused (the text in msg)
inline const char *reach_list_error(const sfa_reach_target_t *t, int32_t n, const TargetModel &m, char *msg, size_t cap) {
    if (n > kReachTargetsMax) {
        snprintf(msg, cap, "%d targets in one list; at most %d", n, kReachTargetsMax);
        return msg;
    }
    for (int32_t k = 0; k < n; ++k) {
        const sfa_reach_target_t &x = t[k];
        const sfa_target_t plain = {x.contig, x.begin, x.end};
        if (target_list_error(&plain, 1, m, msg, cap)) {  // (its words; it numbers the one target it sees 0)
            const char *colon = strchr(msg, ':');
            const std::string tail = colon ? colon : msg;
            snprintf(msg, cap, "target %d%s", k, tail.c_str());
            return msg;
        }
        if (x.lead < 0 || x.lead > kReachLeadMax) {
            snprintf(msg, cap, "target %d: lead %d outside 0 .. %d", k, x.lead, kReachLeadMax);
            return msg;
        }
        if (x.strand != 0 && x.strand != '+' && x.strand != '-') {
            snprintf(msg, cap, "target %d: strand %d is none of 0, '+', '-'", k, static_cast<int>(x.strand));
            return msg;
        }
        if (x.pad[0] || x.pad[1] || x.pad[2]) {
            snprintf(msg, cap, "target %d: the padding is not zero", k);
            return msg;
        }
    }
    return nullptr;
}

// ---- the rule ----
inline bool reach_admits(const sfa_reach_target_t &t, const int32_t contig, const int strand, const int32_t x) {
    if (t.contig != contig || (t.strand != 0 && t.strand != strand)) return false;
    const int64_t b = t.begin, e = t.end, lead = t.lead;
    return strand == '+' ? (b - lead <= x && x < e) : (b <= x && x < e + lead);
}
// the base of target t a read at x (admitted by t) reaches first
inline int32_t reach_anchor_of(const sfa_reach_target_t &t, const int strand, const int32_t x) { return strand == '+' ? std::max(x, t.begin) : std::min(x, t.end - 1); }
// a coordinate anchor of contig offset `off` as an entry of the contig's track
inline int32_t reach_entry_of(const int32_t anchor, const int32_t off) { return anchor < 0 ? kReachNone : (anchor < off ? kReachBelowTrack : anchor - off); }

// The model: mask (target_mask_words words) and anchor COORDINATES ([total_cols], -1: none) of a checked list; returns the
// on-target columns
inline int64_t reach_tables(const sfa_reach_target_t *t, int32_t n, const TargetModel &m, std::vector<uint32_t> *mask, std::vector<int32_t> *anchor) {
    mask->assign(target_mask_words(m.total_cols), 0u);
    anchor->assign(static_cast<size_t>(m.total_cols), kReachNone);
    int64_t on = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        const int strand = m.job_strand[j];
        for (int32_t col = 0; col < m.job_len[j]; ++col) {
            const int32_t x = place_col(strand, col, rl, off);
            bool any = false;
            int32_t best = kReachNone;
            for (int32_t k = 0; k < n; ++k) {
                if (!reach_admits(t[k], contig, strand, x)) continue;
                const int32_t a = reach_anchor_of(t[k], strand, x);
                best = !any ? a : (strand == '+' ? std::min(best, a) : std::max(best, a));
                any = true;
            }
            if (!any) continue;
            const int64_t g = m.col_off[j] + col;
            (*mask)[static_cast<size_t>(g >> 5)] |= 1u << (g & 31);
            (*anchor)[static_cast<size_t>(g)] = best;
            ++on;
        }
    }
    return on;
}

// ---- the prepared form ----
struct ReachRun {
    int32_t lo, hi;   // columns [lo, hi) of the job
    int32_t a, step;  // entry of column j: a + step * j; step 0 and a = kReachBelowTrack: no entry
};
struct ReachPrepared {
    std::vector<int32_t> run_off;  // [n_jobs + 1]: job j's runs are runs[run_off[j] .. run_off[j + 1])
    std::vector<ReachRun> runs;
};

// the run of `runs[0 .. n)` (rising, disjoint) that holds column j, or -1
SFA_ROW_HD int32_t reach_find_run(const ReachRun *runs, const int32_t n, const int32_t j) {
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
SFA_ROW_HD int32_t reach_run_entry(const ReachRun &r, const int32_t j) { return r.a + r.step * j; }

inline void reach_prepare(const sfa_reach_target_t *t, int32_t n, const TargetModel &m, ReachPrepared *p) {
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
    // Along a job the rule is one rule in a RISING coordinate u: u = x on '+', u = -x on '-' (the read goes on towards higher u
    // either way), column = u + shift.  In u a target is a body [B, E) with a lead-in [B - lead, B) whose columns lead to B.
    struct Piece {
        int64_t lo, hi, b;  // [lo, hi) in u, clipped to the job's; b: the body's first u (a lead-in's value)
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
            const sfa_reach_target_t &x = t[order[static_cast<size_t>(q)]];
            if (x.strand != 0 && x.strand != strand) continue;
            const int64_t b = plus ? static_cast<int64_t>(x.begin) : -(static_cast<int64_t>(x.end) - 1);
            const int64_t e = plus ? static_cast<int64_t>(x.end) : -static_cast<int64_t>(x.begin) + 1;
            const Piece bd = {std::max(b, ulo), std::min(e, uhi), b}, ld = {std::max(b - x.lead, ulo), std::min(b, uhi), b};
            if (bd.lo < bd.hi) body.push_back(bd), cut.push_back(bd.lo), cut.push_back(bd.hi);
            if (ld.lo < ld.hi) lead.push_back(ld), cut.push_back(ld.lo), cut.push_back(ld.hi);
        }
        std::sort(cut.begin(), cut.end());
        cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
        const auto by_lo = [](const Piece &x, const Piece &y) { return x.lo < y.lo; };
        std::sort(body.begin(), body.end(), by_lo);
        std::sort(lead.begin(), lead.end(), by_lo);
        // between two cuts the rule is one: inside a body the anchor is the column's own coordinate; else the nearest body in
        // front among the lead-ins that cover the piece (a heap by b: the covering lead-in with the lowest b)
        const auto later = [](const Piece &x, const Piece &y) { return x.b > y.b; };
        std::priority_queue<Piece, std::vector<Piece>, decltype(later)> open(later);
        size_t bi = 0, li = 0;
        int64_t body_hi = ulo;  // the bodies seen so far reach up to here
        const size_t run0 = p->runs.size();
        for (size_t i = 0; i + 1 < cut.size(); ++i) {
            const int64_t lo = cut[i], hi = cut[i + 1];
            while (bi < body.size() && body[bi].lo <= lo) body_hi = std::max(body_hi, body[bi++].hi);
            while (li < lead.size() && lead[li].lo <= lo) open.push(lead[li++]);
            while (!open.empty() && open.top().b <= lo) open.pop();
            ReachRun r = {static_cast<int32_t>(lo + shift), static_cast<int32_t>(hi + shift), 0, 0};
            if (lo < body_hi) {
                r.a = plus ? 0 : rl, r.step = plus ? 1 : -1;
            } else if (!open.empty()) {
                const int64_t coord = plus ? open.top().b : -open.top().b;  // (a target's begin on '+', its end - 1 on '-')
                r.a = reach_entry_of(static_cast<int32_t>(coord), off);
            } else {
                continue;
            }
            if (p->runs.size() > run0 && p->runs.back().hi == r.lo && p->runs.back().a == r.a && p->runs.back().step == r.step)
                p->runs.back().hi = r.hi;
            else
                p->runs.push_back(r);
        }
        p->run_off[static_cast<size_t>(j) + 1] = static_cast<int32_t>(p->runs.size());
    }
}

// The tables the runs give when every column bisects them, as the build kernel does: mask (target_mask_words words) and anchor
// ENTRIES ([total_cols]: an index into the contig's track, kReachNone, kReachBelowTrack); returns the on-target columns
inline int64_t reach_tables_from_runs(const ReachPrepared &p, const TargetModel &m, std::vector<uint32_t> *mask, std::vector<int32_t> *entry) {
    mask->assign(target_mask_words(m.total_cols), 0u);
    entry->assign(static_cast<size_t>(m.total_cols), kReachNone);
    int64_t on = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const ReachRun *runs = p.runs.data() + p.run_off[static_cast<size_t>(j)];
        const int32_t n_runs = p.run_off[static_cast<size_t>(j) + 1] - p.run_off[static_cast<size_t>(j)];
        for (int32_t col = 0; col < m.job_len[j]; ++col) {
            const int32_t r = reach_find_run(runs, n_runs, col);
            if (r < 0) continue;
            const int64_t g = m.col_off[j] + col;
            (*mask)[static_cast<size_t>(g >> 5)] |= 1u << (g & 31);
            (*entry)[static_cast<size_t>(g)] = reach_run_entry(runs[r], col);
            ++on;
        }
    }
    return on;
}

// ---- the live rule under a depth cap: base bit, and the depth of the ANCHOR's entry below the cap (no entry: depth 0) ----
SFA_ROW_HD bool reach_live(const bool base_bit, const uint32_t *track, const int32_t entry, const int32_t track_len, const uint32_t cap) {
    if (!base_bit) return false;
    if (entry < 0 || entry >= track_len) return true;  // (kReachBelowTrack; an entry beyond the track never leaves reach_prepare)
    return track[entry] < cap;
}

// The live mask of a base mask and its entries under depth and cap into `live`; returns the live columns
inline int64_t reach_live_mask(const std::vector<uint32_t> &base, const std::vector<int32_t> &entry, const uint32_t *depth, const int64_t *cov_off, const uint32_t cap,
                               const TargetModel &m, std::vector<uint32_t> *live) {
    live->assign(target_mask_words(m.total_cols), 0u);
    int64_t n_live = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j];
        for (int32_t k = 0; k < m.job_len[j]; ++k) {
            const int64_t g = m.col_off[j] + k;
            const bool bit = (base[static_cast<size_t>(g >> 5)] >> (g & 31)) & 1u;
            if (!reach_live(bit, depth + cov_off[contig], entry[static_cast<size_t>(g)], coverage_track_len(m.ref_len[contig]), cap)) continue;
            (*live)[static_cast<size_t>(g >> 5)] |= 1u << (g & 31);
            ++n_live;
        }
    }
    return n_live;
}

}  // namespace sfa
