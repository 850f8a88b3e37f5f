// sdtw_session_class.hpp -- target classes of a session's slots (sfa_session_classes): the lowest cost among the on-target columns
// of a slot's carried cost row and the lowest among the others, with the columns they stand in.
//
// The rows of a slot's jobs lie back to back without padding (sdtw_session.hpp), so a slot's row is ONE array of total_columns
// floats whose index is the column the mask and the tie rule (target_rules.hpp) count in: the jobs matter only when the winning
// column is placed.  No column outside the slot's own row is read into the reduction.
//   * sdtw_session_class_kernel: block (named slot i, part p) reduces 8192 columns.  A row begins at any alignment: up to three
//     head columns in front of the first 16-byte boundary and up to three tail columns behind the last whole quad are taken one
//     by one (by part 0); the body is read in 16-byte loads, eight in flight per lane.  A quad's four mask bits come from the two
//     mask words it can touch (the mask has one word behind its last); the mask is total_columns / 8 bytes for all slots and
//     stays in cache.  A lane meets its columns in rising order, so `<` keeps the lowest column of equal costs; lanes, waves
//     (through LDS) and parts are merged with class_before, a total order: no float atomics, nothing depends on arrival order.
//   * sdtw_session_class_rows_kernel: one wave per named slot merges the parts, places the two winning columns (class_place) and
//     writes the slot's sfa_class_t.
// Memory-bound: a call reads the named slots' cost rows once (4 bytes per column) and writes 16 bytes per part.
#pragma once

#include <hip/hip_runtime.h>

#include "target_rules.hpp"

namespace sfa {

constexpr int kClassThreads = 256;
constexpr int kClassQuadsPerLane = 8;
constexpr int kClassPartQuads = kClassThreads * kClassQuadsPerLane;  // 2048 quads: 8192 columns per block
constexpr int kClassTailLane = 64;                                   // part 0: lanes 0..2 take the head columns, 64..66 the tail's

// the parts a row of total_cols columns is reduced in (at least one: the head and tail columns are part 0's)
inline int32_t class_parts(int64_t total_cols) { return static_cast<int32_t>(std::max<int64_t>((total_cols / 4 + kClassPartQuads - 1) / kClassPartQuads, 1)); }

struct ClassPartial {  // of a (named slot, part): the best column of either class, kNoColumn while nothing finite was met
    float on_c, off_c;
    int32_t on_g, off_g;
};

struct SessionClassArgs {
    const int32_t *slot;   // [n] slots of the session, none empty or poisoned
    const float *rows;     // column 0 of slot 0's carried cost row
    const uint32_t *mask;  // target_mask_words(total_cols) words
    ClassPartial *part;    // [n][n_parts]
    int64_t total_cols;    // below 2^31
    int32_t n, n_parts;
};

struct SessionClassRowsArgs {
    const ClassPartial *part;
    const int64_t *col_off;  // [n_jobs]
    RefTables ref;
    sfa_class_t *out;        // [n]
    int32_t n, n_parts, n_jobs;
    int32_t first_on, first_off;  // lowest column of either class, -1: the class is empty
};

__global__ void sdtw_session_class_kernel(const SessionClassArgs a);
__global__ void sdtw_session_class_rows_kernel(const SessionClassRowsArgs a);

#ifdef SFA_DEFINE_SESSION_CLASS_KERNELS  // defined in exactly one translation unit (sdtw_inst_session_class.hip)

struct ClassBest {
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

// one column in rising order of the lane: `<` keeps the first of equal costs
__device__ __forceinline__ void class_offer(ClassBest &on, ClassBest &off, const float c, const int32_t g, const bool is_on) {
    const float c_on = is_on ? c : INFINITY, c_off = is_on ? INFINITY : c;
    const bool t_on = c_on < on.c, t_off = c_off < off.c;
    on.c = t_on ? c_on : on.c;
    on.g = t_on ? g : on.g;
    off.c = t_off ? c_off : off.c;
    off.g = t_off ? g : off.g;
}

__global__ void __launch_bounds__(kClassThreads) sdtw_session_class_kernel(const SessionClassArgs a) {
    const int i = blockIdx.x / a.n_parts, part = blockIdx.x - i * a.n_parts;
    if (i >= a.n) return;
    const int tid = threadIdx.x;
    const int32_t total = static_cast<int32_t>(a.total_cols);
    const float *row = a.rows + static_cast<int64_t>(a.slot[i]) * a.total_cols;
    const int32_t to_boundary = static_cast<int32_t>((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3);
    const int32_t head = min(to_boundary, total);
    const int32_t nq = (total - head) >> 2;  // whole quads behind the head, each 16-byte aligned
    const int32_t tail0 = head + 4 * nq;
    ClassBest on{INFINITY, kNoColumn}, off{INFINITY, kNoColumn};
    auto single = [&](const int32_t g) { class_offer(on, off, row[g], g, (a.mask[g >> 5] >> (g & 31)) & 1u); };
    if (part == 0 && tid < head) single(tid);
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
                const int32_t g = head + 4 * q;
                const uint32_t bits = __builtin_amdgcn_alignbit(a.mask[(g >> 5) + 1], a.mask[g >> 5], g & 31);
                class_offer(on, off, v[u].x, g, bits & 1u);
                class_offer(on, off, v[u].y, g + 1, bits & 2u);
                class_offer(on, off, v[u].z, g + 2, bits & 4u);
                class_offer(on, off, v[u].w, g + 3, bits & 8u);
            }
        }
    }
    if (part == 0 && tid >= kClassTailLane && tid - kClassTailLane < total - tail0) single(tail0 + tid - kClassTailLane);
    on.merge_wave();
    off.merge_wave();
    __shared__ ClassPartial lds[kClassThreads / 64];
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
__global__ void __launch_bounds__(64) sdtw_session_class_rows_kernel(const SessionClassRowsArgs a) {
    const int i = blockIdx.x;
    if (i >= a.n) return;
    ClassBest on{INFINITY, kNoColumn}, off{INFINITY, kNoColumn};
    const ClassPartial *p = a.part + static_cast<int64_t>(i) * a.n_parts;
    for (int k = threadIdx.x; k < a.n_parts; k += 64) {
        on.merge(p[k].on_c, p[k].on_g);
        off.merge(p[k].off_c, p[k].off_g);
    }
    on.merge_wave();
    off.merge_wave();
    if (threadIdx.x != 0) return;
    // a class whose every column costs +inf: nothing was less than the initial +inf, and the lowest column of the class wins
    if (on.g == kNoColumn && a.first_on >= 0) on.g = a.first_on;
    if (off.g == kNoColumn && a.first_off >= 0) off.g = a.first_off;
    const ClassPlace pn = class_place(on.g, a.n_jobs, a.col_off, a.ref), pf = class_place(off.g, a.n_jobs, a.col_off, a.ref);
    sfa_class_t r;
    r.on_score = on.c;
    r.off_score = off.c;
    r.on_rid = pn.rid;
    r.on_pos_end = pn.pos_end;
    r.off_rid = pf.rid;
    r.off_pos_end = pf.pos_end;
    r.on_strand = pn.strand;
    r.off_strand = pf.strand;
    r.pad[0] = r.pad[1] = 0;
    r.n_events = 0;  // (the host's: it knows the slots' lengths)
    r.valid = 1;
    a.out[i] = r;
}
#endif

}  // namespace sfa
