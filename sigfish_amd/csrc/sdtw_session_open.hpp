// sdtw_session_open.hpp -- open and closed target groups of a session's slots (sfa_session_open_classes): the lowest cost among
// the columns of a slot's carried cost row whose group is open, and the lowest among the others (closed groups, the background),
// with the columns they stand in and the groups those columns belong to.
//
// Two classes, as in sdtw_session_class.hpp, but the class of a column is not a bit of a mask: it is bit `label` of a bitmap of
// open groups that comes with the call (quota_rules.hpp), the label being the column's entry of the session's label table
// (group_rules.hpp).  Closing a group changes 1 bit of a kernel argument: nothing is rebuilt, nothing is uploaded.
//   * sdtw_session_open_kernel: block (named slot i, part p) reduces 8192 columns, walking the row as the class and the group
//     kernels do (up to three head columns, 16-byte loads with eight in flight per lane, up to three tail columns; head and tail are
//     part 0's).  The bitmap -- kOpenWords = 32 words, normalised by the host so that every bit at or above n_groups is 0 -- arrives
//     in the argument block, is copied into LDS once per block (a chain of selects over the 32 scalar words: indexing the argument
//     block with a lane's index would send it through scratch) and is looked up per column: word label >> 5, bit label & 31.  The
//     background's label n_groups <= 1023 has a word and its bit is 0: no branch per column.  A quad's four labels come from the
//     two 8-byte words it can touch, as in sdtw_session_group_kernel.  A lane keeps (cost, column) per class with `<` and meets
//     its columns in rising order; lanes merge by shuffles, the four waves through LDS, with class_before.  No atomics, no memset.
//   * sdtw_session_open_rows_kernel: one wave per named slot merges the parts (rounds of 64), lane 0 places both winners
//     (class_place), reads their labels and writes the sfa_open_class_t.
// Memory-bound: a call reads the named slots' rows once (4 bytes per column) and the labels (2 bytes per column, shared by all
// slots: from cache), and writes 16 bytes per part.
#pragma once

#include <hip/hip_runtime.h>

#include "quota_rules.hpp"
#include "sdtw_session_class.hpp"

namespace sfa {

struct SessionOpenArgs {
    const int32_t *slot;         // [n] slots of the session, none empty or poisoned
    const float *rows;           // column 0 of slot 0's carried cost row
    const uint64_t *label;       // group_label_words(total_cols) words: four uint16 labels each
    ClassPartial *part;          // [n][n_parts]
    int64_t total_cols;          // below 2^31
    int32_t n, n_parts;
    uint32_t open[kOpenWords];   // normalised (open_normalise): bits at or above n_groups are 0
};

struct SessionOpenRowsArgs {
    const ClassPartial *part;
    const int64_t *col_off;      // [n_jobs]
    RefTables ref;
    const uint16_t *label;       // the label table, one entry per column
    sfa_open_class_t *out;       // [n]
    int32_t n, n_parts, n_jobs;
    int32_t first_on, first_off;  // lowest column of either class under the call's bitmap, -1: the class is empty
};

__global__ void sdtw_session_open_kernel(const SessionOpenArgs a);
__global__ void sdtw_session_open_rows_kernel(const SessionOpenRowsArgs a);

#ifdef SFA_DEFINE_SESSION_OPEN_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_open.hip)

struct OpenBest {
    float c;
    int32_t g;
    __device__ __forceinline__ void merge(const float oc, const int32_t og) {
        const bool take = class_before(oc, og, c, g);
        c = take ? oc : c;
        g = take ? og : g;
    }
    __device__ __forceinline__ void merge_wave() {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) merge(__shfl_xor(c, d, 64), __shfl_xor(g, d, 64));
    }
};

// one column in rising order of the lane: `<` keeps the first of equal costs.  The class: bit `lab` of the block's bitmap
__device__ __forceinline__ void open_offer(OpenBest &on, OpenBest &off, const uint32_t *bitmap, const float c, const int32_t g, const uint32_t lab) {
    const bool is_on = (bitmap[lab >> 5] >> (lab & 31)) & 1u;
    const float c_on = is_on ? c : INFINITY, c_off = is_on ? INFINITY : c;
    const bool t_on = c_on < on.c, t_off = c_off < off.c;
    on.c = t_on ? c_on : on.c;
    on.g = t_on ? g : on.g;
    off.c = t_off ? c_off : off.c;
    off.g = t_off ? g : off.g;
}

__global__ void __launch_bounds__(kClassThreads) sdtw_session_open_kernel(const SessionOpenArgs a) {
    const int i = blockIdx.x / a.n_parts, part = blockIdx.x - i * a.n_parts;
    if (i >= a.n) return;
    const int tid = threadIdx.x;
    __shared__ uint32_t bitmap[kOpenWords];
    __shared__ ClassPartial lds[kClassThreads / 64];
    {
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < kOpenWords; ++k) w = tid == k ? a.open[k] : w;  // (constant indices: scalar registers, no scratch)
        if (tid < kOpenWords) bitmap[tid] = w;
    }
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const float *row = a.rows + static_cast<int64_t>(a.slot[i]) * a.total_cols;
    const int32_t to_boundary = static_cast<int32_t>((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3);
    const int32_t head = min(to_boundary, total);
    const int32_t nq = (total - head) >> 2;  // whole quads behind the head, each 16-byte aligned
    const int32_t tail0 = head + 4 * nq;
    OpenBest on{INFINITY, kNoColumn}, off{INFINITY, kNoColumn};
    const uint16_t *label1 = reinterpret_cast<const uint16_t *>(a.label);
    if (part == 0 && tid < head) open_offer(on, off, bitmap, row[tid], tid, label1[tid]);
    if (nq > 0) {
        const int32_t q0 = part * kClassPartQuads + tid;
        float4 v[kClassQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kClassQuadsPerLane; ++u) {  // (a quad beyond the row's last is read as the last one and not offered)
            const int32_t q = min(q0 + u * kClassThreads, nq - 1);
            v[u] = *reinterpret_cast<const float4 *>(row + head + 4 * static_cast<int64_t>(q));
        }
#pragma unroll
        for (int u = 0; u < kClassQuadsPerLane; ++u) {
            const int32_t q = q0 + u * kClassThreads;
            if (q < nq) {
                const int32_t g = head + 4 * q;  // g & 3 == head: the quad's labels begin 2 * head bytes into a word
                const uint64_t lo = a.label[g >> 2], hi = a.label[(g >> 2) + 1];
                const int sh = 16 * (g & 3);
                const uint64_t labs = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
                open_offer(on, off, bitmap, v[u].x, g, static_cast<uint32_t>(labs & 0xffff));
                open_offer(on, off, bitmap, v[u].y, g + 1, static_cast<uint32_t>((labs >> 16) & 0xffff));
                open_offer(on, off, bitmap, v[u].z, g + 2, static_cast<uint32_t>((labs >> 32) & 0xffff));
                open_offer(on, off, bitmap, v[u].w, g + 3, static_cast<uint32_t>(labs >> 48));
            }
        }
    }
    if (part == 0 && tid >= kClassTailLane && tid - kClassTailLane < total - tail0) {
        const int32_t g = tail0 + tid - kClassTailLane;
        open_offer(on, off, bitmap, row[g], g, label1[g]);
    }
    on.merge_wave();
    off.merge_wave();
    if ((tid & 63) == 0) lds[tid >> 6] = ClassPartial{on.c, off.c, on.g, off.g};
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kClassThreads / 64; ++w) {
            on.merge(lds[w].on_c, lds[w].on_g);
            off.merge(lds[w].off_c, lds[w].off_g);
        }
        a.part[static_cast<int64_t>(i) * a.n_parts + part] = ClassPartial{on.c, off.c, on.g, off.g};
    }
}

// grid: n blocks of one wave
__global__ void __launch_bounds__(64) sdtw_session_open_rows_kernel(const SessionOpenRowsArgs a) {
    const int i = blockIdx.x;
    if (i >= a.n) return;
    OpenBest on{INFINITY, kNoColumn}, off{INFINITY, kNoColumn};
    const ClassPartial *p = a.part + static_cast<int64_t>(i) * a.n_parts;
    for (int k = threadIdx.x; k < a.n_parts; k += 64) {  // (rounds of 64 parts)
        on.merge(p[k].on_c, p[k].on_g);
        off.merge(p[k].off_c, p[k].off_g);
    }
    on.merge_wave();
    off.merge_wave();
    if (threadIdx.x != 0) return;
    // a class whose every column costs +inf: nothing was less than the initial +inf, and the lowest column of the class wins
    if (on.g == kNoColumn && a.first_on >= 0) on.g = a.first_on;
    if (off.g == kNoColumn && a.first_off >= 0) off.g = a.first_off;
    a.out[i] = open_class_record(on.c, on.g, off.c, off.g, a.label, a.n_jobs, a.col_off, a.ref);
}
#endif

}  // namespace sfa
