// sdtw_session_group.hpp -- target groups of a session's slots (sfa_session_group_bests): the lowest cost among the columns of
// every group of a slot's carried cost row, and among the columns of no group, with the columns they stand in.
//
// The row is walked as sdtw_session_class.hpp walks it (one array of total_columns floats at any 4-byte alignment: up to three
// head columns, 16-byte loads with eight in flight per lane, up to three tail columns), but K + 1 = n_groups + 1 accumulators do
// not fit registers.  What is reduced is a column's KEY (group_rules.hpp): (bits of the cost << 32) | column, whose unsigned
// 64-bit minimum is the project's tie rule.  An integer minimum is exact, associative and commutative: no float atomics, and no
// result depends on the order in which lanes, waves or blocks arrive.
//   * sdtw_session_group_kernel: block (named slot i, part p of 8192 columns) keeps K + 1 keys in LDS (at most 8 KB), all-ones at
//     first.  A lane holds one pending (label, key) in registers and folds its columns into it while the label stays the same; on
//     a label change the pending pair goes to LDS (ds_min_u64).  At the end of the walk a wave whose pending labels are all equal
//     reduces its keys by shuffles and lane 0 issues the one LDS minimum; otherwise every lane issues its own.  Runs of one label
//     are thousands of columns long, so the first case is the common one.  A quad's four labels are 8 bytes at a 2-byte
//     alignment: they come from the two 8-byte words the quad can touch, shifted (the table has one word behind its last).
//     After the barrier the block sends the entries it touched -- only those -- to the slot's [K + 1] keys in global memory with
//     global_atomic_umin_x2; the host set that table to all-ones on the same stream.  Nothing is kept per (part, group).
//   * sdtw_session_group_rows_kernel: one wave per named slot; lane k places entries k, k + 64, ... (class_place) into the
//     slot's sfa_group_best_t records; the wave merges the two smallest keys and lane 0 writes the sfa_group_head_t.
// Memory-bound by design: a call reads the named slots' rows once (4 bytes per column) and the labels (2 bytes per column, shared
// by all slots: from cache).
#pragma once

#include <hip/hip_runtime.h>

#include "group_rules.hpp"
#include "sdtw_session_class.hpp"

namespace sfa {

constexpr int kGroupEntriesMax = kGroupMax + 1;  // LDS keys of a block

struct SessionGroupArgs {
    const int32_t *slot;             // [n] slots of the session, none empty or poisoned
    const float *rows;               // column 0 of slot 0's carried cost row
    const uint64_t *label;           // group_label_words(total_cols) words: four uint16 labels each
    unsigned long long *key;         // [n][n_entries], all-ones
    int64_t total_cols;              // below 2^31
    int32_t n, n_parts, n_entries;   // n_entries = n_groups + 1
};

struct SessionGroupRowsArgs {
    const unsigned long long *key;   // [n][n_entries]
    const int64_t *col_off;          // [n_jobs]
    RefTables ref;
    sfa_group_best_t *best;          // [n][n_entries], or nullptr
    sfa_group_head_t *head;          // [n]
    int32_t n, n_entries, n_jobs;
};

__global__ void sdtw_session_group_kernel(const SessionGroupArgs a);
__global__ void sdtw_session_group_rows_kernel(const SessionGroupRowsArgs a);

#ifdef SFA_DEFINE_SESSION_GROUP_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_group.hip)

struct GroupPending {  // of a lane: the smallest key of the columns met since the label last changed; label < 0: none
    int32_t label;
    unsigned long long key;
    __device__ __forceinline__ void flush(unsigned long long *lds) const {
        if (label >= 0) atomicMin(&lds[label], key);
    }
    __device__ __forceinline__ void offer(unsigned long long *lds, const float c, const int32_t g, const int32_t lab) {
        const unsigned long long k = group_key(c, g);
        if (lab != label) {
            flush(lds);
            label = lab;
            key = k;
        } else {
            key = k < key ? k : key;
        }
    }
};

__global__ void __launch_bounds__(kClassThreads) sdtw_session_group_kernel(const SessionGroupArgs a) {
    const int i = blockIdx.x / a.n_parts, part = blockIdx.x - i * a.n_parts;
    if (i >= a.n) return;
    const int tid = threadIdx.x;
    __shared__ unsigned long long lds[kGroupEntriesMax];
    for (int e = tid; e < a.n_entries; e += kClassThreads) lds[e] = kGroupNoKey;
    __syncthreads();
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const float *row = a.rows + static_cast<int64_t>(a.slot[i]) * a.total_cols;
    const int32_t to_boundary = static_cast<int32_t>((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3);
    const int32_t head = min(to_boundary, total);
    const int32_t nq = (total - head) >> 2;  // whole quads behind the head, each 16-byte aligned
    const int32_t tail0 = head + 4 * nq;
    GroupPending pend{-1, kGroupNoKey};
    const uint16_t *label1 = reinterpret_cast<const uint16_t *>(a.label);
    if (part == 0 && tid < head) pend.offer(lds, row[tid], tid, label1[tid]);
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
                pend.offer(lds, v[u].x, g, static_cast<int32_t>(labs & 0xffff));
                pend.offer(lds, v[u].y, g + 1, static_cast<int32_t>((labs >> 16) & 0xffff));
                pend.offer(lds, v[u].z, g + 2, static_cast<int32_t>((labs >> 32) & 0xffff));
                pend.offer(lds, v[u].w, g + 3, static_cast<int32_t>(labs >> 48));
            }
        }
    }
    if (part == 0 && tid >= kClassTailLane && tid - kClassTailLane < total - tail0) {
        const int32_t g = tail0 + tid - kClassTailLane;
        pend.offer(lds, row[g], g, label1[g]);
    }
    // the pending pairs: one LDS minimum per wave when every lane that holds one holds the same label
    const unsigned long long have = __ballot(pend.label >= 0);
    if (have != 0) {
        const int32_t ref = __shfl(pend.label, __ffsll(have) - 1, 64);
        if (__ballot(pend.label >= 0 && pend.label != ref) == 0) {
            unsigned long long k = pend.label >= 0 ? pend.key : kGroupNoKey;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long o = __shfl_xor(k, d, 64);
                k = o < k ? o : k;
            }
            if ((tid & 63) == 0) atomicMin(&lds[ref], k);
        } else {
            pend.flush(lds);
        }
    }
    __syncthreads();
    unsigned long long *out = a.key + static_cast<int64_t>(i) * a.n_entries;
    for (int e = tid; e < a.n_entries; e += kClassThreads) {
        const unsigned long long k = lds[e];
        if (k != kGroupNoKey) atomicMin(&out[e], k);
    }
}

// grid: n blocks of one wave
__global__ void __launch_bounds__(64) sdtw_session_group_rows_kernel(const SessionGroupRowsArgs a) {
    const int i = blockIdx.x;
    if (i >= a.n) return;
    const unsigned long long *key = a.key + static_cast<int64_t>(i) * a.n_entries;
    GroupTop2 t = group_top2_none();
    for (int e = threadIdx.x; e < a.n_entries; e += 64) {
        const uint64_t k = key[e];
        group_top2_offer(t, k, e);
        if (a.best) a.best[static_cast<int64_t>(i) * a.n_entries + e] = group_best_of(k, class_place(group_key_col(k), a.n_jobs, a.col_off, a.ref));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {  // (a lane and its partner hold disjoint sets of entries at every step)
        GroupTop2 o;
        o.k1 = __shfl_xor(static_cast<unsigned long long>(t.k1), d, 64);
        o.k2 = __shfl_xor(static_cast<unsigned long long>(t.k2), d, 64);
        o.e1 = __shfl_xor(t.e1, d, 64);
        o.e2 = __shfl_xor(t.e2, d, 64);
        t = group_top2_merge(t, o);
    }
    if (threadIdx.x == 0) a.head[i] = group_head_of(t);
}
#endif

}  // namespace sfa
