// target_rules.hpp -- the host rules of a session's target classes (sfa_session_targets, sfa_session_classes; pure C++, no HIP,
// no context; tests/c/target_rules.cpp runs them without a GPU):
//   * which columns of a slot's row are ON target (target_mask): one bit per column of the concatenated column space, job after
//     job in the order of the rows' col_off, bit j & 31 of word j >> 5.  Column j of job (contig, strand) is on target when
//     place_col (row_rules.hpp: the coordinate a row reports for an alignment that ends in that column) lies in an interval of the
//     contig.  place_col is strictly monotone in the column, so an interval is a run of columns whose two ends are found by
//     bisection over place_col itself: the mapping is stated in row_rules.hpp only.
//   * what a list of targets is refused for (target_list_error)
//   * how the partial minima of a class are ordered (class_before: lowest cost, then lowest column of the row -- job order, '+'
//     before '-', lowest column within a job) and how the winning column becomes contig, coordinate and strand (class_place)
//   * the decision from a slot's class result (target_decide)
// sdtw_session_class.hpp reduces the rows under the mask with class_before and places the winners with class_place.
#pragma once

#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/sigfish_amd.h"
#include "row_rules.hpp"

namespace sfa {

// What the rules read of the reference model: the jobs in row order and the contigs' lengths and offsets (host memory)
struct TargetModel {
    int32_t num_ref, n_jobs;
    const int32_t *job_contig;  // [n_jobs]
    const int8_t *job_strand;   // [n_jobs] '+' / '-'
    const int32_t *job_len;     // [n_jobs]
    const int64_t *col_off;     // [n_jobs] first column of job j inside a slot's row
    const int32_t *ref_len;     // [num_ref]
    const int32_t *ref_st_offset;
    int64_t total_cols;
};

constexpr int32_t kNoColumn = INT32_MAX;  // the column of a partial minimum nothing was offered to

// words of the mask of a row of total_cols columns, and one more: the kernel reads the word behind a quad's own
inline size_t target_mask_words(int64_t total_cols) { return static_cast<size_t>((total_cols + 31) / 32) + 1; }

// nullptr, or why target k is refused (the text in msg)
inline const char *target_list_error(const sfa_target_t *t, int32_t n, const TargetModel &m, char *msg, size_t cap) {
    for (int32_t k = 0; k < n; ++k) {
        const sfa_target_t &x = t[k];
        if (x.contig < 0 || x.contig >= m.num_ref) {
            snprintf(msg, cap, "target %d: contig %d out of range (the reference has %d)", k, x.contig, m.num_ref);
            return msg;
        }
        if (x.begin < 0) {
            snprintf(msg, cap, "target %d: begin %d is negative", k, x.begin);
            return msg;
        }
        if (x.end <= x.begin) {
            snprintf(msg, cap, "target %d: the interval [%d, %d) is empty", k, x.begin, x.end);
            return msg;
        }
        const int64_t limit = static_cast<int64_t>(m.ref_st_offset[x.contig]) + m.ref_len[x.contig] + 1;
        if (x.end > limit) {
            snprintf(msg, cap, "target %d: end %d lies beyond contig %d (rows report coordinates below %lld)", k, x.end, x.contig, static_cast<long long>(limit));
            return msg;
        }
    }
    return nullptr;
}

// first column in [0, rl] from which on `pred(place_col(column))` holds; pred is false on a prefix and true behind it
template <typename P>
inline int32_t target_first_col(const int strand, const int32_t rl, const int32_t off, P pred) {
    int32_t lo = 0, hi = rl;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (pred(place_col(strand, mid, rl, off)))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The mask of the list (checked by target_list_error) into `mask` (target_mask_words words); returns the on-target columns
inline int64_t target_mask(const sfa_target_t *t, int32_t n, const TargetModel &m, std::vector<uint32_t> *mask) {
    mask->assign(target_mask_words(m.total_cols), 0u);
    for (int32_t j = 0; j < m.n_jobs; ++j) {
        const int32_t contig = m.job_contig[j], rl = m.job_len[j], off = m.ref_st_offset[contig];
        const int strand = m.job_strand[j];
        const bool rising = place_col(strand, 1, rl, off) > place_col(strand, 0, rl, off);
        for (int32_t k = 0; k < n; ++k) {
            if (t[k].contig != contig) continue;
            const int32_t b = t[k].begin, e = t[k].end;
            // columns whose coordinate x has b <= x < e: a run, [first x >= b, first x >= e) along a rising coordinate and
            // [first x < e, first x < b) along a falling one
            const int32_t lo = rising ? target_first_col(strand, rl, off, [&](int x) { return x >= b; }) : target_first_col(strand, rl, off, [&](int x) { return x < e; });
            const int32_t hi = rising ? target_first_col(strand, rl, off, [&](int x) { return x >= e; }) : target_first_col(strand, rl, off, [&](int x) { return x < b; });
            for (int64_t g = m.col_off[j] + lo; g < m.col_off[j] + hi;) {
                const int64_t w = g >> 5, stop = std::min<int64_t>((w + 1) << 5, m.col_off[j] + hi);
                const int nb = static_cast<int>(stop - g), sh = static_cast<int>(g & 31);
                (*mask)[static_cast<size_t>(w)] |= (nb == 32 ? 0xffffffffu : ((1u << nb) - 1u)) << sh;
                g = stop;
            }
        }
    }
    int64_t on = 0;
    for (const uint32_t w : *mask) on += __builtin_popcount(w);
    return on;
}

// the lowest column of the row that is on target (on = true) or off target; -1: the class is empty
inline int32_t target_first_of_class(const std::vector<uint32_t> &mask, int64_t total_cols, bool on) {
    for (int64_t w = 0; w * 32 < total_cols; ++w) {
        uint32_t bits = on ? mask[static_cast<size_t>(w)] : ~mask[static_cast<size_t>(w)];
        if (total_cols - w * 32 < 32) bits &= (1u << (total_cols - w * 32)) - 1u;
        if (bits) return static_cast<int32_t>(w * 32 + __builtin_ctz(bits));
    }
    return -1;
}

// ---- the order of a class's partial minima: lowest cost, then lowest column of the row ----
SFA_ROW_HD bool class_before(const float c, const int32_t col, const float best, const int32_t best_col) { return c < best || (c == best && col < best_col); }

// contig, coordinate and strand of column `col` of a slot's row (kNoColumn or negative: none)
struct ClassPlace {
    int32_t rid, pos_end;
    int8_t strand;
};
SFA_ROW_HD ClassPlace class_place(const int32_t col, const int32_t n_jobs, const int64_t *col_off, const RefTables &t) {
    if (col < 0 || col == kNoColumn) return ClassPlace{-1, -1, 0};
    int32_t lo = 0, hi = n_jobs - 1;  // the last job whose first column is <= col
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (col_off[mid] <= col)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int32_t rid = t.job_contig[lo];
    const int8_t strand = t.job_strand[lo];
    return ClassPlace{rid, place_col(strand, static_cast<int>(col - col_off[lo]), t.ref_len[rid], t.ref_st_offset[rid]), strand};
}

// ---- the decision.  'A' accept, 'U' unblock, 0 none ----
enum { kTargetEnrich = 0, kTargetDeplete = 1 };
// 'T' on target, 'O' off target, 0 undecided
inline char target_class_of(const sfa_class_t &c, const int32_t min_events, const float margin) {
    if (!c.valid || c.n_events < min_events || !(margin >= 0.0f) || !isfinite(margin)) return 0;
    const float on = c.on_rid < 0 ? INFINITY : c.on_score, off = c.off_rid < 0 ? INFINITY : c.off_score;
    if (isinf(on) && isinf(off)) return 0;
    const float need = margin * static_cast<float>(c.n_events);
    if (off - on >= need) return 'T';
    if (on - off >= need) return 'O';
    return 0;
}
inline char target_decide(const sfa_class_t &c, const int mode, const int32_t min_events, const float margin) {
    if (mode != kTargetEnrich && mode != kTargetDeplete) return 0;
    const char cls = target_class_of(c, min_events, margin);
    if (!cls) return 0;
    return ((cls == 'T') == (mode == kTargetEnrich)) ? 'A' : 'U';
}

}  // namespace sfa
