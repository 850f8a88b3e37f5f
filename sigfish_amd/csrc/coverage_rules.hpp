// coverage_rules.hpp -- the host rules of a session's coverage cap (sfa_session_coverage_config / _add / _depth; pure C++, no HIP,
// no context; tests/c/coverage_rules.cpp runs them without a GPU).  The mask, place_col and TargetModel are target_rules.hpp's and
// row_rules.hpp's; nothing of them is restated here.
//   * the depth layout: one uint32 per coordinate a row of the contig can report.  Contig c has ref_len[c] + 1 entries, entry
//     x - ref_st_offset[c] stands for coordinate x; the contigs lie back to back from cov_off[c] (coverage_offsets).  Both strands
//     of a contig share the track: depth belongs to the position, not to the strand.
//   * what a list of intervals is refused for (coverage_list_error: target_list_error, word for word).  A list that passes may
//     still begin below ref_st_offset -- no row reports such a coordinate, so that part of an interval counts nowhere
//     (coverage_span clips to the track; the add kernel and the host model both go through it).
//   * the live rule (coverage_live): column j of job (contig, strand) is live when its bit of the base mask is set AND the depth
//     of the coordinate place_col gives it lies below the cap.  A coordinate closes on both strands at once.
//   * the whole step on the host (coverage_live_mask): base mask + depth + cap -> live mask and its popcount; the lowest column of
//     either class under it is target_first_of_class's.
// sdtw_session_cover.hpp adds the intervals to the tracks and derives the live mask with the same two functions.
#pragma once

#include "target_rules.hpp"

namespace sfa {

constexpr int32_t kCoverCapMax = 1 << 30;        // the largest cap
constexpr int32_t kCoverIntervalsMax = 1 << 20;  // intervals of one sfa_session_coverage_add call

// entries of contig c's track
SFA_ROW_HD int32_t coverage_track_len(const int32_t ref_len) { return ref_len + 1; }

// cov_off[0 .. num_ref]: where every contig's track begins; the last entry is the number of entries of all tracks
inline void coverage_offsets(const int32_t *ref_len, const int32_t num_ref, std::vector<int64_t> *cov_off) {
    cov_off->assign(static_cast<size_t>(num_ref) + 1, 0);
    for (int32_t c = 0; c < num_ref; ++c) (*cov_off)[static_cast<size_t>(c) + 1] = (*cov_off)[static_cast<size_t>(c)] + coverage_track_len(ref_len[c]);
}

// bytes the feature adds to a session: the tracks and the second mask
inline size_t coverage_bytes(const int64_t track_entries, const int64_t total_cols) { return 4 * static_cast<size_t>(track_entries) + 4 * target_mask_words(total_cols); }

// nullptr, or why interval k is refused (the text in msg): the conditions of a target list
inline const char *coverage_list_error(const sfa_target_t *iv, int32_t n, const TargetModel &m, char *msg, size_t cap) { return target_list_error(iv, n, m, msg, cap); }

// the entries [lo, hi) of a contig's track that the interval [begin, end) of coordinates covers (empty: lo >= hi)
struct CoverSpan {
    int32_t lo, hi;
};
SFA_ROW_HD CoverSpan coverage_span(const int32_t begin, const int32_t end, const int32_t rl, const int32_t off) {
    const int64_t lo = static_cast<int64_t>(begin) - off, hi = static_cast<int64_t>(end) - off, len = coverage_track_len(rl);
    return CoverSpan{static_cast<int32_t>(lo < 0 ? 0 : (lo > len ? len : lo)), static_cast<int32_t>(hi < 0 ? 0 : (hi > len ? len : hi))};
}

// the track entry of column j of a job: place_col's coordinate, counted from the contig's offset (0 .. rl for j in [0, rl])
SFA_ROW_HD int32_t coverage_entry(const int strand, const int32_t j, const int32_t rl, const int32_t off) { return place_col(strand, j, rl, off) - off; }

// ---- the live rule.  base_bit: the column's bit of the base mask; track: the contig's track (depth + cov_off[contig]) ----
SFA_ROW_HD bool coverage_live(const bool base_bit, const uint32_t *track, const int strand, const int32_t j, const int32_t rl, const int32_t off, const uint32_t cap) {
    return base_bit && track[coverage_entry(strand, j, rl, off)] < cap;
}

// depth += 1 over every interval of the list (checked by coverage_list_error), as the add kernel leaves it
inline void coverage_add(const sfa_target_t *iv, int32_t n, const TargetModel &m, const int64_t *cov_off, uint32_t *depth) {
    for (int32_t k = 0; k < n; ++k) {
        const CoverSpan s = coverage_span(iv[k].begin, iv[k].end, m.ref_len[iv[k].contig], m.ref_st_offset[iv[k].contig]);
        for (int32_t e = s.lo; e < s.hi; ++e) ++depth[cov_off[iv[k].contig] + e];
    }
}

// The live mask of a base mask (target_mask_words words) under depth and cap into `live`; returns the live columns
inline int64_t coverage_live_mask(const std::vector<uint32_t> &base, const uint32_t *depth, const int64_t *cov_off, const uint32_t cap, const TargetModel &m,
                                  std::vector<uint32_t> *live) {
    live->assign(target_mask_words(m.total_cols), 0u);
    int64_t n_live = 0;
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.ref_len[contig], off = m.ref_st_offset[contig];
        for (int32_t k = 0; k < m.job_len[j]; ++k) {
            const int64_t g = m.col_off[j] + k;
            const bool bit = (base[static_cast<size_t>(g >> 5)] >> (g & 31)) & 1u;
            if (!coverage_live(bit, depth + cov_off[contig], m.job_strand[j], k, rl, off, cap)) continue;
            (*live)[static_cast<size_t>(g >> 5)] |= 1u << (g & 31);
            ++n_live;
        }
    }
    return n_live;
}

}  // namespace sfa
