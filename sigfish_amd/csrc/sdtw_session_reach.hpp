// sdtw_session_reach.hpp -- reach targets of a session (sfa_session_targets_reach): the base mask and the anchor table on the
// device, and the live mask of a reach session under a depth cap (reach_rules.hpp states the rule, the prepared runs and the
// live rule; nothing of them is restated here).  Both kernels have the geometry of session_cover_mask_kernel
// (sdtw_session_cover.hpp): one lane per column of a slot's row, 64 columns per wave, 256 per block; the job of the block's
// first column by a block-uniform bisection over col_off, a lane walks on from there; the 64 answers of a wave through a ballot
// into two mask words that lanes 0 and 32 store; columns at or beyond total_cols answer 0, so the spare word behind the row is
// written as zero or not at all (the buffer is zeroed in front of the launch); the stats the host wants -- columns of the class
// and the lowest column of either class, a CoverStats record -- merged per block through LDS and then by integer atomics.
//   * session_reach_build_kernel: a lane finds the run of its column by bisection over its job's runs (reach_find_run) and
//     stores the run's entry (reach_run_entry), or kReachNone, into the anchor table: one int32 per column, consecutive lanes
//     store consecutive words.
//   * session_reach_live_kernel: a lane reads its bit of the base mask and its anchor and evaluates reach_live on the anchor's
//     entry of the contig's track.  It differs from session_cover_mask_kernel in what it reads the depth AT, by one 4-byte read
//     per column; inside a body the anchors of a wave are one contiguous run of the track as there, and a whole lead-in reads one
//     entry.
// Plain C++ and vector stores; memory-bound and tiny beside a sweep.
#pragma once

#include <hip/hip_runtime.h>

#include "reach_rules.hpp"
#include "sdtw_session_cover.hpp"

namespace sfa {

struct SessionReachBuildArgs {
    const ReachRun *runs;     // reach_prepare's, job after job
    const int32_t *run_off;   // [n_jobs + 1]
    const int64_t *col_off;   // [n_jobs]
    uint32_t *mask;           // target_mask_words(total_cols) words
    int32_t *anchor;          // [total_cols]
    CoverStats *stats;        // live: the on-target columns
    int64_t total_cols;       // below 2^31
    int32_t n_jobs, n_words;  // n_words: target_mask_words(total_cols)
};

struct SessionReachLiveArgs {
    const uint32_t *base;     // target_mask_words(total_cols) words
    const int32_t *anchor;    // [total_cols]
    uint32_t *live;           // as many words as base
    const uint32_t *depth;
    const int64_t *cov_off;   // [num_ref + 1]
    const int64_t *col_off;   // [n_jobs]
    RefTables ref;
    CoverStats *stats;
    int64_t total_cols;       // below 2^31
    int32_t n_jobs, n_words;
    uint32_t cap;
};

__global__ void session_reach_build_kernel(const SessionReachBuildArgs a);
__global__ void session_reach_live_kernel(const SessionReachLiveArgs a);

#ifdef SFA_DEFINE_SESSION_REACH_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_reach.hip)

// the last job whose first column is <= col0: the same for every lane of the block
__device__ __forceinline__ int32_t reach_block_job(const int64_t *col_off, const int32_t n_jobs, const int32_t col0) {
    int32_t lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (col_off[mid] <= col0)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the wave's 64 answers into its two words of `out` (lanes 0 and 32), and the block's stats into the record
__device__ __forceinline__ void reach_store_and_count(const bool on, const bool inside, const int32_t col0, uint32_t *out, const uint32_t *and_with, const int32_t n_words,
                                                      CoverStats *stats) {
    const int tid = threadIdx.x;
    const unsigned long long bits = __ballot(on), valid = __ballot(inside);
    const int lane = tid & 63, wave = tid >> 6;
    const int32_t wcol0 = col0 + 64 * wave;  // the wave's first column: a multiple of 64, so its two words are 32-bit aligned
    if ((lane & 31) == 0) {
        const int32_t w = (wcol0 >> 5) + (lane >> 5);
        if (w < n_words) out[w] = (and_with ? and_with[w] : 0xffffffffu) & static_cast<uint32_t>(bits >> (lane & 32));
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
        if (s.live) atomicAdd(&stats->live, s.live);
        if (s.first_on != kNoColumn) atomicMin(&stats->first_on, s.first_on);
        if (s.first_off != kNoColumn) atomicMin(&stats->first_off, s.first_off);
    }
}

// grid: cover_mask_blocks(total_cols) blocks
__global__ void __launch_bounds__(kCoverThreads) session_reach_build_kernel(const SessionReachBuildArgs a) {
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kCoverThreads;  // (below total: the grid is cover_mask_blocks)
    const int32_t job0 = reach_block_job(a.col_off, a.n_jobs, col0);
    const int32_t col = col0 + static_cast<int32_t>(threadIdx.x);
    const bool inside = col < total;
    bool on = false;
    if (inside) {
        int32_t job = job0;
        while (job + 1 < a.n_jobs && a.col_off[job + 1] <= col) ++job;
        const int32_t j = col - static_cast<int32_t>(a.col_off[job]), r0 = a.run_off[job];
        const int32_t r = reach_find_run(a.runs + r0, a.run_off[job + 1] - r0, j);
        on = r >= 0;
        a.anchor[col] = on ? reach_run_entry(a.runs[r0 + r], j) : kReachNone;
    }
    reach_store_and_count(on, inside, col0, a.mask, nullptr, a.n_words, a.stats);
}

// grid: cover_mask_blocks(total_cols) blocks
__global__ void __launch_bounds__(kCoverThreads) session_reach_live_kernel(const SessionReachLiveArgs a) {
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kCoverThreads;  // (below total: the grid is cover_mask_blocks)
    const int32_t job0 = reach_block_job(a.col_off, a.n_jobs, col0);
    const int32_t col = col0 + static_cast<int32_t>(threadIdx.x);
    const bool inside = col < total;
    bool live = false;
    if (inside) {
        int32_t job = job0;
        while (job + 1 < a.n_jobs && a.col_off[job + 1] <= col) ++job;
        const int32_t contig = a.ref.job_contig[job];
        const bool bit = (a.base[col >> 5] >> (col & 31)) & 1u;
        live = reach_live(bit, a.depth + a.cov_off[contig], a.anchor[col], coverage_track_len(a.ref.ref_len[contig]), a.cap);
    }
    reach_store_and_count(live, inside, col0, a.live, a.base, a.n_words, a.stats);
}
#endif

}  // namespace sfa
