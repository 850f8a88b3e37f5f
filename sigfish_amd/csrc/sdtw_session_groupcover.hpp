// sdtw_session_groupcover.hpp -- group caps of a session (sfa_session_group_coverage_config / sfa_session_group_coverage): the live
// label table derived from the base table and the depth tracks, and the depth record of every group (group_cover_rules.hpp states
// the rules, coverage_rules.hpp the track's layout; nothing of them is restated here).  The add kernel is sdtw_session_cover.hpp's.
// Both kernels share one geometry: a lane owns kGroupCoverCols = 4 consecutive columns of a slot's row -- one 8-byte word of a label
// table -- a wave 256 columns, a block of 256 lanes 1024.  The job of the block's first column is found by a block-uniform
// bisection over col_off; a lane walks on from there, column by column, so a quad that straddles a job boundary is handled per
// column (with jobs of thousands of columns that is no step or one).  The depth entry of a column rises with the column on '+' and
// falls with it on '-', so a wave reads one contiguous run of a track either way.
//   * session_cover_label_kernel: reads the quad's base labels as one 8-byte word, turns each into group_live_label and stores the
//     quad as one 8-byte word; the quad that holds the row's last column (and only it) may reach beyond the row, and is stored
//     column by column, two bytes each, so that nothing beyond the row is written.  A background column reads no depth.  The
//     lowest live column of every label is kept in an int32[n_groups + 1] table in LDS, set to kNoColumn: a lane offers a column
//     with an LDS atomicMin where the label differs from the one before it in its quad (labels come in runs), and after the barrier
//     the touched entries are merged into the global table with atomicMin.  The global table was reset to kNoColumn by the launch
//     in front (an upload of at most 4 KB); integer minima do not depend on arrival order.
//   * session_cover_group_kernel: the records over the '+' jobs' columns (group_cover_counts) by BASE label.  A lane sums the run of
//     equal labels in its quad in registers and flushes it into the block's tables in LDS -- columns and capped 32-bit, sum 64-bit,
//     minimum, maximum: 24 bytes per entry, 24 KB at 1024 entries -- with LDS atomics; after the barrier the entries that hold a
//     column are merged into the global records with integer atomics (atomicAdd on 64 bits, atomicMin / atomicMax on 32).  The
//     global records were reset to group_cover_none by the launch in front.
// Both are memory-bound and tiny beside a sweep: 2 + 2 bytes per column and 4 per labelled column for the first, 2 bytes per
// column and 4 per '+' column for the second.
#pragma once

#include <hip/hip_runtime.h>

#include "group_cover_rules.hpp"

namespace sfa {

constexpr int kGroupCoverThreads = 256;
constexpr int kGroupCoverCols = 4;                                     // columns of a lane: one 8-byte word of labels
constexpr int kGroupCoverSpan = kGroupCoverThreads * kGroupCoverCols;  // columns of a block

struct SessionCoverLabelArgs {
    const uint64_t *base;     // group_label_words(total_cols) words of four labels
    uint16_t *live;           // as many; the words behind the row hold the background and are never written
    const uint32_t *depth;
    const int64_t *cov_off;   // [num_ref + 1]
    const int64_t *col_off;   // [n_jobs]
    RefTables ref;
    int32_t *first;           // [n_groups + 1], reset to kNoColumn in front of the launch
    int64_t total_cols;       // below 2^31
    int32_t n_jobs, n_groups;
    uint32_t cap;
};

struct SessionCoverGroupArgs {
    const uint64_t *base;
    const uint32_t *depth;
    const int64_t *cov_off;
    const int64_t *col_off;
    RefTables ref;
    sfa_group_cover_t *rec;   // [n_groups + 1], reset to group_cover_none in front of the launch
    int64_t total_cols;
    int32_t n_jobs, n_groups;
    uint32_t cap;
};

// blocks of either launch: every column of the row, kGroupCoverSpan per block
inline int32_t group_cover_blocks(int64_t total_cols) { return static_cast<int32_t>((total_cols + kGroupCoverSpan - 1) / kGroupCoverSpan); }

__global__ void session_cover_label_kernel(const SessionCoverLabelArgs a);
__global__ void session_cover_group_kernel(const SessionCoverGroupArgs a);

#ifdef SFA_DEFINE_SESSION_GROUPCOVER_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_groupcover.hip)

// the last job whose first column is <= col0: the same for every lane of the block
__device__ __forceinline__ int32_t group_cover_first_job(const int64_t *col_off, const int32_t n_jobs, const int32_t col0) {
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

// grid: group_cover_blocks(total_cols) blocks
__global__ void __launch_bounds__(kGroupCoverThreads) session_cover_label_kernel(const SessionCoverLabelArgs a) {
    __shared__ int32_t first[kGroupMax + 1];
    const int tid = threadIdx.x;
    const int32_t entries = a.n_groups + 1;
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads) first[e] = kNoColumn;
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kGroupCoverSpan;  // (below total: the grid is group_cover_blocks)
    int32_t job = group_cover_first_job(a.col_off, a.n_jobs, col0);
    const int32_t c0 = col0 + kGroupCoverCols * tid;
    if (c0 < total) {
        const uint16_t bg = static_cast<uint16_t>(a.n_groups);
        const uint64_t word = a.base[c0 >> 2];  // (the table has a word behind the row's last: in bounds for every c0 < total)
        uint64_t out = 0;
        int32_t prev = -1;
#pragma unroll
        for (int k = 0; k < kGroupCoverCols; ++k) {
            const int32_t col = c0 + k;
            uint16_t l = static_cast<uint16_t>(word >> (16 * k));
            if (col < total) {
                while (job + 1 < a.n_jobs && a.col_off[job + 1] <= col) ++job;
                if (l != bg) {
                    const int32_t contig = a.ref.job_contig[job];
                    l = group_live_label(l, a.depth + a.cov_off[contig], a.ref.job_strand[job], col - static_cast<int32_t>(a.col_off[job]), a.ref.ref_len[contig],
                                         a.ref.ref_st_offset[contig], a.cap, bg);
                }
                if (static_cast<int32_t>(l) != prev) atomicMin(&first[l], col);  // (columns rise inside the quad: a run's first column is enough)
                prev = l;
            }
            out |= static_cast<uint64_t>(l) << (16 * k);
        }
        if (c0 + kGroupCoverCols <= total) {
            *reinterpret_cast<uint64_t *>(a.live + c0) = out;  // (c0 is a multiple of 4: 8-byte aligned)
        } else {
            for (int k = 0; c0 + k < total; ++k) a.live[c0 + k] = static_cast<uint16_t>(out >> (16 * k));  // the row's last quad: nothing beyond the row
        }
    }
    __syncthreads();
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads)
        if (first[e] != kNoColumn) atomicMin(a.first + e, first[e]);
}

// grid: group_cover_blocks(total_cols) blocks
__global__ void __launch_bounds__(kGroupCoverThreads) session_cover_group_kernel(const SessionCoverGroupArgs a) {
    __shared__ unsigned long long s_sum[kGroupMax + 1];
    __shared__ uint32_t s_cols[kGroupMax + 1], s_capped[kGroupMax + 1], s_min[kGroupMax + 1], s_max[kGroupMax + 1];
    const int tid = threadIdx.x;
    const int32_t entries = a.n_groups + 1;
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads) s_sum[e] = 0ull, s_cols[e] = 0u, s_capped[e] = 0u, s_min[e] = UINT32_MAX, s_max[e] = 0u;
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kGroupCoverSpan;
    int32_t job = group_cover_first_job(a.col_off, a.n_jobs, col0);
    const int32_t c0 = col0 + kGroupCoverCols * tid;
    if (c0 < total) {
        const uint64_t word = a.base[c0 >> 2];
        sfa_group_cover_t run = group_cover_none();  // of the run of equal labels the lane is in
        int32_t run_label = -1;
        const auto flush = [&]() {
            if (run_label < 0 || run.columns == 0) return;
            atomicAdd(&s_cols[run_label], static_cast<uint32_t>(run.columns));
            if (run.capped) atomicAdd(&s_capped[run_label], static_cast<uint32_t>(run.capped));
            if (run.depth_sum) atomicAdd(&s_sum[run_label], static_cast<unsigned long long>(run.depth_sum));
            atomicMin(&s_min[run_label], run.depth_min);
            atomicMax(&s_max[run_label], run.depth_max);
        };
#pragma unroll
        for (int k = 0; k < kGroupCoverCols; ++k) {
            const int32_t col = c0 + k;
            if (col >= total) break;
            while (job + 1 < a.n_jobs && a.col_off[job + 1] <= col) ++job;
            const int strand = a.ref.job_strand[job];
            if (!group_cover_counts(strand)) continue;
            const int32_t label = static_cast<int32_t>(static_cast<uint16_t>(word >> (16 * k)));
            if (label != run_label) {
                flush();
                run = group_cover_none();
                run_label = label;
            }
            const int32_t contig = a.ref.job_contig[job];
            const uint32_t d = a.depth[a.cov_off[contig] + coverage_entry(strand, col - static_cast<int32_t>(a.col_off[job]), a.ref.ref_len[contig], a.ref.ref_st_offset[contig])];
            group_cover_note(run, d, a.cap);
        }
        flush();
    }
    __syncthreads();
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads) {
        if (s_cols[e] == 0u) continue;
        sfa_group_cover_t *r = a.rec + e;
        atomicAdd(reinterpret_cast<unsigned long long *>(&r->columns), static_cast<unsigned long long>(s_cols[e]));
        if (s_capped[e]) atomicAdd(reinterpret_cast<unsigned long long *>(&r->capped), static_cast<unsigned long long>(s_capped[e]));
        if (s_sum[e]) atomicAdd(reinterpret_cast<unsigned long long *>(&r->depth_sum), s_sum[e]);
        atomicMin(&r->depth_min, s_min[e]);
        atomicMax(&r->depth_max, s_max[e]);
    }
}
#endif

}  // namespace sfa
