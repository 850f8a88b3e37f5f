// group_cover_rules.hpp -- the host rules of a session's group cap (sfa_session_group_coverage_config / sfa_session_group_coverage;
// pure C++, no HIP, no context; tests/c/group_cover_rules.cpp runs them without a GPU).  The labels and their table are
// group_rules.hpp's, the depth layout, coverage_entry and coverage_offsets are coverage_rules.hpp's, place_col and TargetModel are
// row_rules.hpp's and target_rules.hpp's; nothing of them is restated here.
//   * the live label (group_live_label): the live label of column j of job (contig, strand) is its base label -- group_labels'
//     own: the lowest group id that covers it -- while the depth of the coordinate the column reports lies below the group cap,
//     and the background, n_groups, from then on.  A background column stays background whatever its depth.  A column covered by
//     groups 3 and 7 whose coordinate is capped goes to the background, NOT to group 7: the cap closes the coordinate, it does not
//     uncover a group underneath.  The group cap is a number of its own, independent of the mask's cap (coverage_rules.hpp); both
//     read the one depth track of the session.
//   * the label firsts: the lowest column of every live label 0 .. n_groups, kNoColumn for a label without live columns.  While a
//     group cap is set these, not open_label_firsts of the base table, are what open_first_cols is fed (group_cover_firsts_for_open
//     turns kNoColumn into its -1).
//   * the group depth record (sfa_group_cover_t) of every entry 0 .. n_groups: over the columns of the '+' JOBS ONLY whose BASE label
//     is the entry -- columns, those with depth >= cap (capped), the sum, minimum and maximum of their depths.  A forward row
//     reports coordinates off .. off + rl - 1, each once, so every coordinate a forward row reports is counted exactly once; the
//     one coordinate per contig that only the '-' row reports, off + rl, is left out.  An entry without columns: 0, 0, 0,
//     UINT32_MAX, 0 (group_cover_none).
//   * the whole step on the host (group_cover_live_labels, group_cover_records): what the kernels of sdtw_session_groupcover.hpp
//     must give.
#pragma once

#include "coverage_rules.hpp"
#include "group_rules.hpp"

namespace sfa {

constexpr int32_t kGroupCapMax = kCoverCapMax;  // the largest group cap: the mask cap's limit

// bytes a group cap adds to a session beside the depth tracks: the second label table, the firsts and the records of the device
inline size_t group_cover_bytes(const int64_t total_cols, const int32_t n_groups) {
    return 8 * group_label_words(total_cols) + (4 + sizeof(sfa_group_cover_t)) * (static_cast<size_t>(n_groups) + 1);
}

// ---- the live label.  base: the column's label of the base table; track: the contig's track (depth + cov_off[contig]) ----
SFA_ROW_HD uint16_t group_live_label(const uint16_t base, const uint32_t *track, const int strand, const int32_t j, const int32_t rl, const int32_t off, const uint32_t cap,
                                     const uint16_t bg) {
    return (base != bg && track[coverage_entry(strand, j, rl, off)] < cap) ? base : bg;
}

// ---- the record.  One column of depth d into r ----
SFA_ROW_HD sfa_group_cover_t group_cover_none() { return sfa_group_cover_t{0, 0, 0, UINT32_MAX, 0}; }
SFA_ROW_HD void group_cover_note(sfa_group_cover_t &r, const uint32_t d, const uint32_t cap) {
    ++r.columns;
    r.capped += d >= cap;
    r.depth_sum += d;
    r.depth_min = d < r.depth_min ? d : r.depth_min;
    r.depth_max = d > r.depth_max ? d : r.depth_max;
}
// does a job's columns count in the records?  ('+' only: see above)
SFA_ROW_HD bool group_cover_counts(const int strand) { return strand == '+'; }

// what open_first_cols reads: -1 for a label without columns
inline void group_cover_firsts_for_open(const int32_t *first, const int32_t n_groups, std::vector<int32_t> *out) {
    out->resize(static_cast<size_t>(n_groups) + 1);
    for (int32_t g = 0; g <= n_groups; ++g) (*out)[static_cast<size_t>(g)] = first[g] == kNoColumn ? -1 : first[g];
}

// The live table of a base table (4 * group_label_words entries, as group_labels leaves it) under depth and cap into `live` (as
// many entries, the padding holds the background) and the lowest column of every live label into `first` (n_groups + 1 entries,
// kNoColumn: none); returns the columns whose live label is a group
inline int64_t group_cover_live_labels(const std::vector<uint16_t> &base, const uint32_t *depth, const int64_t *cov_off, const uint32_t cap, const int32_t n_groups,
                                       const TargetModel &m, std::vector<uint16_t> *live, std::vector<int32_t> *first) {
    const uint16_t bg = static_cast<uint16_t>(n_groups);
    live->assign(4 * group_label_words(m.total_cols), bg);
    first->assign(static_cast<size_t>(n_groups) + 1, kNoColumn);
    int64_t in = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        for (int32_t k = 0; k < m.job_len[j]; ++k) {
            const int64_t g = m.col_off[j] + k;
            const uint16_t l = group_live_label(base[static_cast<size_t>(g)], depth + cov_off[contig], m.job_strand[j], k, rl, off, cap, bg);
            (*live)[static_cast<size_t>(g)] = l;
            if ((*first)[l] == kNoColumn) (*first)[l] = static_cast<int32_t>(g);  // (columns in rising order)
            in += l != bg;
        }
    }
    return in;
}

// The records of the n_groups + 1 entries from the base table, the depth and the cap
inline void group_cover_records(const std::vector<uint16_t> &base, const uint32_t *depth, const int64_t *cov_off, const uint32_t cap, const int32_t n_groups, const TargetModel &m,
                                std::vector<sfa_group_cover_t> *rec) {
    rec->assign(static_cast<size_t>(n_groups) + 1, group_cover_none());
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        if (!group_cover_counts(m.job_strand[j])) continue;
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        for (int32_t k = 0; k < m.job_len[j]; ++k)
            group_cover_note((*rec)[base[static_cast<size_t>(m.col_off[j] + k)]], depth[cov_off[contig] + coverage_entry(m.job_strand[j], k, rl, off)], cap);
    }
}

}  // namespace sfa
