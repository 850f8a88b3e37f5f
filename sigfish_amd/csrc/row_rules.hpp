// row_rules.hpp -- how a read's partial results become a result row: the reference's update_aln and the tail of dtw_single
// (src/sigfish.c:575-626, 969-983).  ONE statement of it for every finalize kernel (sdtw_kernels.hpp, sdtw_strips.hpp,
// sdtw_session.hpp), the sweeps that keep a candidate list in LDS, the library's host code and tests/c/row_rules.cpp: no HIP in it.
//   * a partial top-2 is merged into the running one in processing order, a later candidate wins ties (Top2Merge over merge_top2)
//   * the sorted list of the 5 best candidates, aln[0] worst .. aln[4] best, in LDS words (top5_offer) and in registers (Top5)
//   * contig, strand and mapq of the winner (primary_row), strand flip and offset (place_row), the rows behind it (secondary_row)
//   * the row of a read with nothing to report (no_row)
// On the device everything is inlined and every array index is a constant once the loops are unrolled: the lists stay in registers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFA_ROW_HD __host__ __device__ __forceinline__
#define SFA_ROW_UNROLL _Pragma("unroll")
#else
#define SFA_ROW_HD inline
#define SFA_ROW_UNROLL
#endif

namespace sfa {

// One result row per read, POD mirror of sfa_result_t (include/sigfish_amd.h; sfa_ctx.hpp holds the two against each other).
struct ResultRow {
    int32_t rid, pos_st, pos_end;
    float score, score2;
    int8_t strand;
    uint8_t mapq, valid, pad;
};
static_assert(sizeof(ResultRow) == 24 && offsetof(ResultRow, rid) == 0 && offsetof(ResultRow, pos_st) == 4 && offsetof(ResultRow, pos_end) == 8 &&
                  offsetof(ResultRow, score) == 12 && offsetof(ResultRow, score2) == 16 && offsetof(ResultRow, strand) == 20 &&
                  offsetof(ResultRow, mapq) == 21 && offsetof(ResultRow, valid) == 22 && offsetof(ResultRow, pad) == 23,
              "the row the C-ABI hands out");

// The empty row: a read without events, a screened-out read, a rank nobody asked for.
SFA_ROW_HD ResultRow no_row() { return ResultRow{-1, -1, -1, INFINITY, INFINITY, 0, 0, 0, 0}; }

SFA_ROW_HD int32_t row_bits(const float f) {
    int32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
SFA_ROW_HD float row_float(const int32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// src/sigfish.c:979-983: (int)round(500*(score2-score)/score) with x86 cvttsd2si saturation, cap 60, store u8
SFA_ROW_HD uint8_t mapq_from_scores(float score, float score2) {
    const float v = 500.0f * (score2 - score) / score;
    const float r = roundf(v);  // == round((double)v) for float inputs
    int q;
    if (!(r >= -2147483648.0f && r < 2147483648.0f))
        q = INT32_MIN;
    else
        q = static_cast<int>(r);
    if (q > 60) q = 60;
    return static_cast<uint8_t>(q);
}

// One partial top-2 (b, s2) merged into the running (best, second), partials in processing order: the second smallest of the
// four stays, and a later partial wins ties (src/sigfish.c:577-583).  True when b is the new best.
SFA_ROW_HD bool merge_top2(float &best, float &second, const float b, const float s2) {
    const float hi = fmaxf(best, b);
    const float lo2 = fminf(second, s2);
    const bool take = !(b > best);
    second = fminf(hi, lo2);  // second smallest of {best, second, b, s2}
    if (take) best = b;
    return take;
}
// The running merge with what the caller keeps of the best partial (Pay: a few ints -- end and job and chunk, end and start and job)
template <typename Pay>
struct Top2Merge {
    float best = INFINITY, second = INFINITY;
    Pay pay;  // of the best partial so far
    SFA_ROW_HD explicit Top2Merge(const Pay &none) : pay(none) {}
    SFA_ROW_HD bool offer(const float b, const float s2, const Pay &p) {
        const bool take = merge_top2(best, second, b, s2);
        if (take) pay = p;
        return take;
    }
};

// The whole sorted candidate list of the reference (SECONDARY_CAP = 5, src/sigfish.h:41), for secondary mappings.  aln[0] is the
// worst entry, aln[4] the best; the insertion is update_aln's (src/sigfish.c:575-594), so the LATER of two equal candidates ranks
// higher and aln[4] is the top-2's winner.  In LDS: 5 x (score bits, two payload words) per read slot, touched by the owner lane
// once per window -- the 32-row fill has no VGPRs to spare for it.
constexpr int kTop5Words = 15;
SFA_ROW_HD void top5_init(int *t5) {
    for (int l = 0; l < 5; ++l) {
        t5[3 * l] = row_bits(INFINITY);
        t5[3 * l + 1] = -1;
        t5[3 * l + 2] = -1;
    }
}
SFA_ROW_HD void top5_offer(int *t5, float sc, int pos, int job) {
    int l = 0;
    while (l < 5 && !(sc > row_float(t5[3 * l]))) ++l;
    if (l == 0) return;
    for (int m = 0; m + 1 < l; ++m) {
        t5[3 * m] = t5[3 * m + 3];
        t5[3 * m + 1] = t5[3 * m + 4];
        t5[3 * m + 2] = t5[3 * m + 5];
    }
    t5[3 * (l - 1)] = row_bits(sc);
    t5[3 * (l - 1) + 1] = pos;
    t5[3 * (l - 1) + 2] = job;
}

// The same list in registers, with P payload words per entry; the LAST one says that the entry is there (>= 0: a job, an index).
// The entries that are not strictly better than the candidate form a prefix of the sorted list; they move down by one and the
// candidate takes the last place of the prefix.
template <int P>
struct Top5 {
    float sc[5];
    int pay[P][5];
    SFA_ROW_HD Top5() {
        SFA_ROW_UNROLL
        for (int m = 0; m < 5; ++m) {
            sc[m] = INFINITY;
            for (int q = 0; q < P; ++q) pay[q][m] = -1;
        }
    }
    template <typename... I>
    SFA_ROW_HD void offer(const float s, const I... p) {
        static_assert(sizeof...(I) == P, "one value per payload word");
        const int v[P] = {p...};
        int l = 0;
        SFA_ROW_UNROLL
        for (int m = 0; m < 5; ++m) l += !(s > sc[m]) ? 1 : 0;
        SFA_ROW_UNROLL
        for (int m = 0; m < 5; ++m) {
            const bool nxt = m + 1 < l, put = m == l - 1;
            const int mn = m < 4 ? m + 1 : 4;
            sc[m] = nxt ? sc[mn] : (put ? s : sc[m]);
            for (int q = 0; q < P; ++q) pay[q][m] = nxt ? pay[q][mn] : (put ? v[q] : pay[q][m]);
        }
    }
    // rank k (0: the best) is the reference's aln[4 - k]; ranks behind the list score +inf
    SFA_ROW_HD float score(const int k) const { return k < 5 ? sc[4 - k] : INFINITY; }
    // the payload of rank k, -1 unless its entry is there and its score finite; returns the rank's score as it stands
    template <typename... I>
    SFA_ROW_HD float rank(const int k, I &...p) const {
        static_assert(sizeof...(I) == P, "one place per payload word");
        const bool ok = pay[P - 1][4 - k] >= 0 && isfinite(sc[4 - k]);
        int q = 0;
        ((p = ok ? pay[q++][4 - k] : -1), ...);
        return sc[4 - k];
    }
};

// The four tables of the reference model a row needs: contig and strand of a job, length and offset of a contig.
struct RefTables {
    const int32_t *job_contig;  // [n_jobs]
    const int8_t *job_strand;   // [n_jobs] '+' / '-'
    const int32_t *ref_len;     // [num_ref]
    const int32_t *ref_st_offset;
};

// Positions of a row from the columns its alignment starts and ends in: strand flip and offset (src/sigfish.c:971-975)
// One column of a strand's array as the coordinate a row reports for it: '-' counts from the contig's other end.  The column an
// alignment ENDS in becomes pos_end on '+' and pos_st on '-' (target_rules.hpp classes a column by this coordinate).
SFA_ROW_HD int place_col(const int strand, const int col, const int rl, const int off) { return ((strand == '+') ? col : rl - col) + off; }
SFA_ROW_HD void place_row(ResultRow &r, const int st, const int end, const int rl, const int off) {
    r.pos_st = place_col(r.strand, (r.strand == '+') ? st : end, rl, off);
    r.pos_end = place_col(r.strand, (r.strand == '+') ? end : st, rl, off);
}
SFA_ROW_HD void place_row(ResultRow &r, const int st, const int end, const RefTables &t) { place_row(r, st, end, t.ref_len[r.rid], t.ref_st_offset[r.rid]); }
// SFA_SESSION_NO_START: no start column was carried, so the coordinate that needs it is -1
SFA_ROW_HD void drop_start(ResultRow &r) { (r.strand == '+' ? r.pos_st : r.pos_end) = -1; }

// The row of a read that was aligned: scores, and contig, strand and mapq when a window won (job >= 0); positions are place_row's
SFA_ROW_HD ResultRow primary_row(const float best, const float second, const int job, const RefTables &t) {
    ResultRow r = no_row();
    r.valid = 1;
    r.score = best;
    r.score2 = second;
    if (job >= 0) {
        r.rid = t.job_contig[job];
        r.strand = t.job_strand[job];
        r.mapq = mapq_from_scores(best, second);
    }
    return r;
}
// The row of a candidate behind the winner: score2 is the next rank's score, mapq 0 (minimap2's convention for secondaries)
SFA_ROW_HD ResultRow secondary_row(const float score, const float next_score, const int job, const int st, const int end, const RefTables &t) {
    ResultRow r = no_row();
    r.valid = 1;
    r.rid = t.job_contig[job];
    r.strand = t.job_strand[job];
    r.score = score;
    r.score2 = next_score;
    place_row(r, st, end, t);
    return r;
}

// Secondary mappings of a batch, both routes (sdtw_sec_finalize_kernel, sdtw_strip_sec_finalize_kernel).  Before pass 2: a read's
// n_lists stored lists of (score bits, end, job), `stride` words apart, offered in processing order, each worst entry first and empty
// entries skipped -- update_aln over all windows -- and rank k of read i written to [k * n + i] of the rank arrays.
SFA_ROW_HD void ranks_from_lists(const int32_t *lists, const int n_lists, const int64_t stride, int32_t *s_job, int32_t *s_col, float *s_score,
                                 const int64_t n, const int64_t i) {
    Top5<2> t;
    for (int j = 0; j < n_lists; ++j)
        for (int e = 0; e < 5; ++e) {
            const int32_t *w = lists + j * stride + 3 * e;
            if (w[2] >= 0) t.offer(row_float(w[0]), w[1], w[2]);
        }
    SFA_ROW_UNROLL
    for (int k = 0; k < 5; ++k) s_score[k * n + i] = t.rank(k, s_col[k * n + i], s_job[k * n + i]);
}
// Behind pass 2: the row of rank k (1..4) of read i from those arrays and the columns traced for it; no_row() where the rank is not
// wanted or not there.
SFA_ROW_HD ResultRow row_from_ranks(const int k, const bool wanted, const int32_t *s_job, const float *s_score, const int64_t n, const int64_t i,
                                    const int32_t *st, const int32_t *end, const RefTables &t) {
    const int job = wanted ? s_job[k * n + i] : -1;
    if (job < 0) return no_row();
    return secondary_row(s_score[k * n + i], k < 4 ? s_score[(k + 1) * n + i] : INFINITY, job, *st, *end, t);
}

// How many reference columns an alignment spans, in sixteenths of its query length: the bucket of the histogram the next batch's
// pass 2 sizes its head start by (the last one open), -1 for no alignment
constexpr int kSpanBuckets = 32;
SFA_ROW_HD int span_bucket(const int st, const int end, const int64_t qlen) {
    if (st < 0 || end < st || qlen <= 0) return -1;
    const int64_t b = (static_cast<int64_t>(end - st + 1) * 16) / qlen;
    return b < kSpanBuckets - 1 ? static_cast<int>(b) : kSpanBuckets - 1;
}

}  // namespace sfa
