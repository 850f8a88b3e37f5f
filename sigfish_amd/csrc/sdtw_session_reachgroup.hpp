// sdtw_session_reachgroup.hpp -- reach groups of a session (sfa_session_target_groups_reach): the label table and its anchors on
// the device, the live labels of a reach label table under a group cap, and the groups' depth records over the body columns
// (reach_group_rules.hpp states the rules, the prepared runs, the live rule and the body test; nothing of them is restated here).
// All three kernels have the geometry of session_cover_label_kernel (sdtw_session_groupcover.hpp): a lane owns kGroupCoverCols = 4
// consecutive columns of a slot's row -- one 8-byte word of a label table, 16 bytes of anchors -- a block of 256 lanes 1024; the
// job of the block's first column by a block-uniform bisection over col_off, a lane walks on from there, column by column, so a
// quad that straddles a job boundary is handled per column.
//   * session_reach_label_build_kernel: per column a bisection over the job's runs (reach_group_find_run); the quad's labels
//     leave as one 8-byte word, its anchors as one 16-byte word.  The quad that holds the row's last column (and only it) may
//     reach beyond the row and is stored column by column, so nothing beyond the row is written: the words behind the row keep
//     the background the host put there.  The lowest column of every label is reduced as session_cover_label_kernel reduces it:
//     an int32[n_groups + 1] table in LDS, an LDS atomicMin where a label differs from the one before it in the quad, the touched
//     entries merged into the global table (reset to kNoColumn in front of the launch) with atomicMin.
//   * session_reach_label_live_kernel: per column the base label (one 8-byte read per quad) and, for a labelled column, its
//     anchor and reach_group_live_label on the anchor's entry of the contig's track; stores and `first` as above.  It differs
//     from session_cover_label_kernel in what it reads the depth AT, by one 4-byte read per labelled column.
//   * session_reach_label_group_kernel: session_cover_group_kernel's records over the columns reach_group_counts admits.
// Plain C++, vector stores, integer atomics; memory-bound and tiny beside a sweep.
#pragma once

#include <hip/hip_runtime.h>

#include "reach_group_rules.hpp"
#include "sdtw_session_groupcover.hpp"

namespace sfa {

struct SessionReachLabelBuildArgs {
    const ReachGroupRun *runs;  // reach_group_prepare's, job after job
    const int32_t *run_off;     // [n_jobs + 1]
    const int64_t *col_off;     // [n_jobs]
    uint16_t *label;            // group_label_words(total_cols) words of four labels; the words behind the row hold the background
    int32_t *anchor;            // [total_cols]
    int32_t *first;             // [n_groups + 1], reset to kNoColumn in front of the launch
    int64_t total_cols;         // below 2^31
    int32_t n_jobs, n_groups;
};

struct SessionReachLabelLiveArgs {
    const uint64_t *base;       // group_label_words(total_cols) words of four labels
    const int32_t *anchor;      // [total_cols]
    uint16_t *live;             // as many words as base; the words behind the row hold the background and are never written
    const uint32_t *depth;
    const int64_t *cov_off;     // [num_ref + 1]
    const int64_t *col_off;     // [n_jobs]
    RefTables ref;
    int32_t *first;             // [n_groups + 1], reset to kNoColumn in front of the launch
    int64_t total_cols;         // below 2^31
    int32_t n_jobs, n_groups;
    uint32_t cap;
};

struct SessionReachLabelGroupArgs {
    const uint64_t *base;
    const int32_t *anchor;
    const uint32_t *depth;
    const int64_t *cov_off;
    const int64_t *col_off;
    RefTables ref;
    sfa_group_cover_t *rec;     // [n_groups + 1], reset to group_cover_none in front of the launch
    int64_t total_cols;
    int32_t n_jobs, n_groups;
    uint32_t cap;
};

__global__ void session_reach_label_build_kernel(const SessionReachLabelBuildArgs a);
__global__ void session_reach_label_live_kernel(const SessionReachLabelLiveArgs a);
__global__ void session_reach_label_group_kernel(const SessionReachLabelGroupArgs a);

#ifdef SFA_DEFINE_SESSION_REACHGROUP_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_reachgroup.hip)

// the last job whose first column is <= col0: the same for every lane of the block
__device__ __forceinline__ int32_t reach_group_first_job(const int64_t *col_off, const int32_t n_jobs, const int32_t col0) {
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

// the quad's labels into the table: one 8-byte word, or column by column in the row's last quad (nothing beyond the row)
__device__ __forceinline__ void reach_group_store_labels(uint16_t *table, const int32_t c0, const int32_t total, const uint64_t out) {
    if (c0 + kGroupCoverCols <= total) {
        *reinterpret_cast<uint64_t *>(table + c0) = out;  // (c0 is a multiple of 4: 8-byte aligned)
    } else {
        for (int k = 0; c0 + k < total; ++k) table[c0 + k] = static_cast<uint16_t>(out >> (16 * k));
    }
}

// grid: group_cover_blocks(total_cols) blocks
__global__ void __launch_bounds__(kGroupCoverThreads) session_reach_label_build_kernel(const SessionReachLabelBuildArgs a) {
    __shared__ int32_t first[kGroupMax + 1];
    const int tid = threadIdx.x;
    const int32_t entries = a.n_groups + 1;
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads) first[e] = kNoColumn;
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kGroupCoverSpan;  // (below total: the grid is group_cover_blocks)
    int32_t job = reach_group_first_job(a.col_off, a.n_jobs, col0);
    const int32_t c0 = col0 + kGroupCoverCols * tid;
    if (c0 < total) {
        const int32_t bg = a.n_groups;
        uint64_t out = 0;
        int4 entry = make_int4(kReachNone, kReachNone, kReachNone, kReachNone);
        int32_t prev = -1;
#pragma unroll
        for (int k = 0; k < kGroupCoverCols; ++k) {
            const int32_t col = c0 + k;
            int32_t l = bg, e = kReachNone;
            if (col < total) {
                while (job + 1 < a.n_jobs && a.col_off[job + 1] <= col) ++job;
                const int32_t j = col - static_cast<int32_t>(a.col_off[job]), r0 = a.run_off[job];
                const int32_t r = reach_group_find_run(a.runs + r0, a.run_off[job + 1] - r0, j);
                if (r >= 0) {
                    const ReachGroupRun run = a.runs[r0 + r];
                    l = run.label;
                    e = reach_group_run_entry(run, j);
                }
                if (l != prev) atomicMin(&first[l], col);  // (columns rise inside the quad: a run's first column is enough)
                prev = l;
            }
            out |= static_cast<uint64_t>(static_cast<uint16_t>(l)) << (16 * k);
            (k == 0 ? entry.x : k == 1 ? entry.y : k == 2 ? entry.z : entry.w) = e;
        }
        reach_group_store_labels(a.label, c0, total, out);
        if (c0 + kGroupCoverCols <= total) {
            *reinterpret_cast<int4 *>(a.anchor + c0) = entry;  // (c0 is a multiple of 4: 16-byte aligned)
        } else {  // the row's last quad: nothing beyond the row
            a.anchor[c0] = entry.x;
            if (c0 + 1 < total) a.anchor[c0 + 1] = entry.y;
            if (c0 + 2 < total) a.anchor[c0 + 2] = entry.z;
        }
    }
    __syncthreads();
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads)
        if (first[e] != kNoColumn) atomicMin(a.first + e, first[e]);
}

// grid: group_cover_blocks(total_cols) blocks
__global__ void __launch_bounds__(kGroupCoverThreads) session_reach_label_live_kernel(const SessionReachLabelLiveArgs a) {
    __shared__ int32_t first[kGroupMax + 1];
    const int tid = threadIdx.x;
    const int32_t entries = a.n_groups + 1;
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads) first[e] = kNoColumn;
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kGroupCoverSpan;  // (below total: the grid is group_cover_blocks)
    int32_t job = reach_group_first_job(a.col_off, a.n_jobs, col0);
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
                    l = reach_group_live_label(l, a.depth + a.cov_off[contig], a.anchor[col], coverage_track_len(a.ref.ref_len[contig]), a.cap, bg);
                }
                if (static_cast<int32_t>(l) != prev) atomicMin(&first[l], col);  // (columns rise inside the quad: a run's first column is enough)
                prev = l;
            }
            out |= static_cast<uint64_t>(l) << (16 * k);
        }
        reach_group_store_labels(a.live, c0, total, out);
    }
    __syncthreads();
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads)
        if (first[e] != kNoColumn) atomicMin(a.first + e, first[e]);
}

// grid: group_cover_blocks(total_cols) blocks
__global__ void __launch_bounds__(kGroupCoverThreads) session_reach_label_group_kernel(const SessionReachLabelGroupArgs a) {
    __shared__ unsigned long long s_sum[kGroupMax + 1];
    __shared__ uint32_t s_cols[kGroupMax + 1], s_capped[kGroupMax + 1], s_min[kGroupMax + 1], s_max[kGroupMax + 1];
    const int tid = threadIdx.x;
    const int32_t entries = a.n_groups + 1;
    for (int32_t e = tid; e < entries; e += kGroupCoverThreads) s_sum[e] = 0ull, s_cols[e] = 0u, s_capped[e] = 0u, s_min[e] = UINT32_MAX, s_max[e] = 0u;
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const int32_t col0 = static_cast<int32_t>(blockIdx.x) * kGroupCoverSpan;
    int32_t job = reach_group_first_job(a.col_off, a.n_jobs, col0);
    const int32_t c0 = col0 + kGroupCoverCols * tid;
    if (c0 < total) {
        const uint64_t word = a.base[c0 >> 2];
        const int32_t bg = a.n_groups;
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
            const int32_t label = static_cast<int32_t>(static_cast<uint16_t>(word >> (16 * k)));
            if (!group_cover_counts(strand) || label == bg) continue;  // (a background column has no anchor: it is no body column)
            const int32_t contig = a.ref.job_contig[job];
            const int32_t entry = a.anchor[col];
            if (!reach_group_counts(strand, entry, col - static_cast<int32_t>(a.col_off[job]), a.ref.ref_len[contig], a.ref.ref_st_offset[contig])) continue;
            if (label != run_label) {
                flush();
                run = group_cover_none();
                run_label = label;
            }
            group_cover_note(run, a.depth[a.cov_off[contig] + entry], a.cap);
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
