// quota_rules.hpp -- the host rules of a session's open and closed target groups (sfa_session_open_classes; pure C++, no HIP, no
// context; tests/c/quota_rules.cpp runs them without a GPU).  The labels, place_col, class_place, class_before and TargetModel are
// group_rules.hpp's and target_rules.hpp's; nothing of them is restated here.
//   * the open bitmap: open_words(n_groups) words of 32 bits, bit g & 31 of word g >> 5 set: group g is open (still wanted).  Bits
//     at or above n_groups are ignored, a null bitmap says every group is open.  open_normalise writes the kOpenWords words the
//     kernel reads: the caller's bits below n_groups, zeros above -- so the background, label n_groups <= 1023, reads as closed
//     without a branch of its own (open_bit on the normalised words IS the class rule).
//   * the class of a column: ON when its label is a group whose bit is set, OFF otherwise (the background, every closed group).
//     The label is group_labels' own: a column covered by several groups follows the lowest id's bit only.
//   * ties: class_before (lowest cost, then lowest column of the row), a total order.  A class without columns: +inf, rid -1,
//     pos -1, strand 0, group -1; a class whose every column costs +inf yields its lowest column (open_first_cols finds the lowest
//     column of either class under a bitmap from the lowest column of every label: n_groups + 1 steps per call, on the host).
//   * the record of a slot from its row (open_class_of_row: the per-column statement the kernel is tested against)
//   * the quota book: a quota and an accepted count per group and the bitmap; host arithmetic only
// sdtw_session_open.hpp reduces the rows under the labels and the normalised bitmap.
#pragma once

#include "group_rules.hpp"

namespace sfa {

constexpr int kOpenWords = (kGroupMax + 1 + 31) / 32;  // 32 words, 128 bytes: every label 0 .. 1023 has a bit

inline int32_t open_words(const int32_t n_groups) { return (n_groups + 31) / 32; }

// the kOpenWords words a kernel reads: bits below n_groups from `open` (all set when open is null), every other bit 0
inline void open_normalise(const uint32_t *open, const int32_t n_groups, uint32_t *out) {
    for (int w = 0; w < kOpenWords; ++w) {
        const int32_t lo = 32 * w, left = n_groups - lo;  // groups this word has bits for
        const uint32_t keep = left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : ((1u << left) - 1u));
        out[w] = keep ? (open ? open[w] : 0xffffffffu) & keep : 0u;  // (keep != 0: w < open_words(n_groups), a word the caller has)
    }
}

// the class rule on normalised words: label in 0 .. 1023
SFA_ROW_HD bool open_bit(const uint32_t *norm, const int32_t label) { return (norm[label >> 5] >> (label & 31)) & 1u; }

// the lowest column of every label (n_groups + 1 entries, -1: the label has no column)
inline void open_label_firsts(const uint16_t *label, const int64_t total_cols, const int32_t n_groups, std::vector<int32_t> *first) {
    first->assign(static_cast<size_t>(n_groups) + 1, -1);
    for (int64_t c = 0; c < total_cols; ++c)
        if ((*first)[label[c]] < 0) (*first)[label[c]] = static_cast<int32_t>(c);
}

// the lowest column of the ON class and of the OFF class under normalised words (-1: the class is empty)
inline void open_first_cols(const std::vector<int32_t> &first, const int32_t n_groups, const uint32_t *norm, int32_t *first_on, int32_t *first_off) {
    int32_t on = -1, off = -1;
    for (int32_t g = 0; g <= n_groups; ++g) {
        const int32_t c = first[static_cast<size_t>(g)];
        if (c < 0) continue;
        int32_t &into = open_bit(norm, g) ? on : off;
        if (into < 0 || c < into) into = c;
    }
    *first_on = on;
    *first_off = off;
}

// what a slot that is empty or poisoned answers
inline sfa_open_class_t open_class_none() {
    sfa_open_class_t r{};
    r.cls.on_score = r.cls.off_score = INFINITY;
    r.cls.on_rid = r.cls.on_pos_end = r.cls.off_rid = r.cls.off_pos_end = -1;
    r.on_group = r.off_group = -1;
    return r;
}

// The record from the two winning columns (kNoColumn: the class is empty) -- the rows kernel's last step and the host's
SFA_ROW_HD sfa_open_class_t open_class_record(const float on_c, const int32_t on_g, const float off_c, const int32_t off_g, const uint16_t *label, const int32_t n_jobs,
                                              const int64_t *col_off, const RefTables &ref) {
    const ClassPlace pn = class_place(on_g, n_jobs, col_off, ref), pf = class_place(off_g, n_jobs, col_off, ref);
    sfa_open_class_t r;
    r.cls.on_score = on_c;
    r.cls.off_score = off_c;
    r.cls.on_rid = pn.rid;
    r.cls.on_pos_end = pn.pos_end;
    r.cls.off_rid = pf.rid;
    r.cls.off_pos_end = pf.pos_end;
    r.cls.on_strand = pn.strand;
    r.cls.off_strand = pf.strand;
    r.cls.pad[0] = r.cls.pad[1] = 0;
    r.cls.n_events = 0;  // (the host's: it knows the slots' lengths)
    r.cls.valid = 1;
    r.on_group = on_g == kNoColumn ? -1 : static_cast<int32_t>(label[on_g]);
    r.off_group = off_g == kNoColumn ? -1 : static_cast<int32_t>(label[off_g]);
    return r;
}

// The record of a row, column by column: what the kernels must give (the columns in rising order, so class_before's second
// clause never fires and `<` alone keeps the lowest column of equal costs; a class of +inf columns keeps its first column)
inline sfa_open_class_t open_class_of_row(const float *row, const uint16_t *label, const int64_t total_cols, const int32_t n_groups, const uint32_t *open, const int32_t n_jobs,
                                          const int64_t *col_off, const RefTables &ref) {
    uint32_t norm[kOpenWords];
    open_normalise(open, n_groups, norm);
    float c[2] = {INFINITY, INFINITY};
    int32_t g[2] = {kNoColumn, kNoColumn};
    for (int64_t col = 0; col < total_cols; ++col) {
        const int k = open_bit(norm, label[col]) ? 0 : 1;
        if (g[k] == kNoColumn || class_before(row[col], static_cast<int32_t>(col), c[k], g[k])) c[k] = row[col], g[k] = static_cast<int32_t>(col);
    }
    return open_class_record(c[0], g[0], c[1], g[1], label, n_jobs, col_off, ref);
}

// ---- the quota book: who has enough.  No device calls, no files ----
class QuotaBook {
   public:
    QuotaBook(const int32_t n_groups, const int64_t quota) : n_groups_(n_groups), quota_(static_cast<size_t>(n_groups), quota), count_(static_cast<size_t>(n_groups), 0) {
        bits_.resize(static_cast<size_t>(open_words(n_groups)));
        open_normalise(nullptr, n_groups, all_);
        std::copy(all_, all_ + bits_.size(), bits_.begin());
    }
    int32_t n_groups() const { return n_groups_; }
    void set_quota(const int32_t group, const int64_t quota) { quota_[static_cast<size_t>(group)] = quota; }  // 0: unlimited
    int64_t quota(const int32_t group) const { return quota_[static_cast<size_t>(group)]; }
    int64_t accepted(const int32_t group) const { return count_[static_cast<size_t>(group)]; }
    bool is_open(const int32_t group) const { return group >= 0 && group < n_groups_ && ((bits_[static_cast<size_t>(group) >> 5] >> (group & 31)) & 1u); }
    const uint32_t *open() const { return bits_.data(); }  // open_words(n_groups) words
    int32_t n_words() const { return static_cast<int32_t>(bits_.size()); }
    // one accepted read of `group` (anything else -- the background, -1 -- is not a group's and counts nowhere): true when the
    // bitmap changed, that is when this read closed the group
    bool note_accept(const int32_t group) {
        if (group < 0 || group >= n_groups_) return false;
        const size_t g = static_cast<size_t>(group);
        ++count_[g];
        if (quota_[g] <= 0 || count_[g] < quota_[g] || !is_open(group)) return false;
        bits_[g >> 5] &= ~(1u << (group & 31));
        return true;
    }

   private:
    int32_t n_groups_;
    std::vector<int64_t> quota_, count_;
    std::vector<uint32_t> bits_;
    uint32_t all_[kOpenWords];
};

}  // namespace sfa
