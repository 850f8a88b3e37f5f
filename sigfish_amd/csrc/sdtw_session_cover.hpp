// sdtw_session_cover.hpp -- coverage caps of a session (sfa_session_coverage_config / _add): a depth track per contig on the
// device and the live mask derived from it (coverage_rules.hpp states the layout and the rule; nothing of them is restated here).
//   * session_cover_add_kernel: block k adds 1 over interval k's entries of its contig's track (coverage_span clips the interval
//     to the track, so no entry outside it is touched).  Lanes stride over the span with atomicAdd on unsigned int: the intervals
//     of a call overlap each other freely and integer adds commute, so the result does not depend on arrival order.
//   * session_cover_mask_kernel: one lane per column of a slot's row, 64 columns per wave, 256 per block.  The job of the block's
//     first column is found by a block-uniform bisection over col_off; a lane walks on from there (with 256 columns per block and
//     jobs of thousands of columns that is no step or one).  The lane evaluates coverage_live -- its depth entry rises with the
//     lane on '+' and falls with it on '-', so a wave reads one contiguous run of the track either way -- and a wave ballot turns
//     the 64 answers into two words; lanes 0 and 32 store `base & bits`.  Columns at or beyond total_cols answer 0, so the spare
//     word behind the row (target_mask_words) is written as zero or not at all (the buffer is zeroed when it is allocated).
//     What the host needs of the new mask -- the live columns and the lowest column of either class (the class kernel's rows
//     step wants them) -- is merged per block through LDS and then by integer atomics into one CoverStats record, which the
//     launch before (a 16-byte upload of its initial value) has reset: integer add and min, nothing depends on arrival order.
// Both kernels are memory-bound and tiny beside a sweep: the add touches 4 bytes per covered base, the mask reads 4 bytes per
// on-target column and writes one bit per column.
#pragma once

#include <hip/hip_runtime.h>

#include "coverage_rules.hpp"

namespace sfa {

constexpr int kCoverThreads = 256;

struct CoverStats {  // of one mask launch; reset to {0, kNoColumn, kNoColumn} in front of it
    unsigned long long live;      // live columns
    int32_t first_on, first_off;  // lowest live column, lowest column that is not live (kNoColumn: none)
};

struct SessionCoverAddArgs {
    const sfa_target_t *iv;   // [n], checked by coverage_list_error
    const int64_t *cov_off;   // [num_ref + 1]
    const int32_t *ref_len;   // [num_ref]
    const int32_t *ref_st_offset;
    uint32_t *depth;          // cov_off[num_ref] entries
    int32_t n;
};

struct SessionCoverMaskArgs {
    const uint32_t *base;     // target_mask_words(total_cols) words
    uint32_t *live;           // as many
    const uint32_t *depth;
    const int64_t *cov_off;   // [num_ref + 1]
    const int64_t *col_off;   // [n_jobs]
    RefTables ref;
    CoverStats *stats;
    int64_t total_cols;       // below 2^31
    int32_t n_jobs, n_words;  // n_words: target_mask_words(total_cols)
    uint32_t cap;
};

// blocks of the mask launch: every column of the row, 256 per block
inline int32_t cover_mask_blocks(int64_t total_cols) { return static_cast<int32_t>((total_cols + kCoverThreads - 1) / kCoverThreads); }

__global__ void session_cover_add_kernel(const SessionCoverAddArgs a);
__global__ void session_cover_mask_kernel(const SessionCoverMaskArgs a);

#ifdef SFA_DEFINE_SESSION_COVER_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_cover.hip)

// grid: n blocks
__global__ void __launch_bounds__(kCoverThreads) session_cover_add_kernel(const SessionCoverAddArgs a) {
    const int k = blockIdx.x;
    if (k >= a.n) return;
    const sfa_target_t iv = a.iv[k];
    const CoverSpan s = coverage_span(iv.begin, iv.end, a.ref_len[iv.contig], a.ref_st_offset[iv.contig]);
    uint32_t *track = a.depth + a.cov_off[iv.contig];
    for (int32_t e = s.lo + static_cast<int32_t>(threadIdx.x); e < s.hi; e += kCoverThreads) atomicAdd(track + e, 1u);
}

// grid: cover_mask_blocks(total_cols) blocks
__global__ void __launch_bounds__(kCoverThreads) session_cover_mask_kernel(const SessionCoverMaskArgs a) {
    const int tid = threadIdx.x;
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kCoverThreads;  // (below total: the grid is cover_mask_blocks)
    // the last job whose first column is <= col0: the same for every lane of the block
    int32_t lo = 0, hi = a.n_jobs - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (a.col_off[mid] <= col0)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int32_t col = col0 + tid;
    const bool inside = col < total;
    bool live = false;
    if (inside) {
        int32_t job = lo;
        while (job + 1 < a.n_jobs && a.col_off[job + 1] <= col) ++job;
        const int32_t contig = a.ref.job_contig[job];
        const bool bit = (a.base[col >> 5] >> (col & 31)) & 1u;
        live = coverage_live(bit, a.depth + a.cov_off[contig], a.ref.job_strand[job], col - static_cast<int32_t>(a.col_off[job]), a.ref.ref_len[contig],
                             a.ref.ref_st_offset[contig], a.cap);
    }
    const unsigned long long bits = __ballot(live), valid = __ballot(inside);
    const int lane = tid & 63, wave = tid >> 6;
    const int32_t wcol0 = col0 + 64 * wave;  // the wave's first column: a multiple of 64, so its two words are 32-bit aligned
    if ((lane & 31) == 0) {
        const int32_t w = (wcol0 >> 5) + (lane >> 5);
        if (w < a.n_words) a.live[w] = a.base[w] & static_cast<uint32_t>(bits >> (lane & 32));
    }
    __shared__ CoverStats lds[kCoverThreads / 64];
    if (lane == 0) {
        const unsigned long long off_bits = valid & ~bits;
        lds[wave] = CoverStats{static_cast<unsigned long long>(__popcll(bits)), bits ? wcol0 + __ffsll(bits) - 1 : kNoColumn,
                               off_bits ? wcol0 + __ffsll(off_bits) - 1 : kNoColumn};
    }
    __syncthreads();
    if (tid == 0) {
        CoverStats s = lds[0];
#pragma unroll
        for (int w = 1; w < kCoverThreads / 64; ++w) {
            s.live += lds[w].live;
            s.first_on = min(s.first_on, lds[w].first_on);
            s.first_off = min(s.first_off, lds[w].first_off);
        }
        if (s.live) atomicAdd(&a.stats->live, s.live);
        if (s.first_on != kNoColumn) atomicMin(&a.stats->first_on, s.first_on);
        if (s.first_off != kNoColumn) atomicMin(&a.stats->first_off, s.first_off);
    }
}
#endif

}  // namespace sfa
