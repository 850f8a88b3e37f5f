// sdtw_session.hpp -- alignment sessions: a read's subsequence DTW extended as its events arrive (sfa_session_extend).
//
// Dependencies of the recurrence (src/cdtw.c:171-189) flow downwards and to the right only, so the LAST query row of a (read,
// contig, strand) sweep is all the rows below it need: one f32 per reference column, plus one i32 per column when the start
// column of every cell is propagated forwards (the rule of pass 2 and of the row strips, sdtw_strips.hpp).  A session keeps
// that row per slot (a growing read) in HBM between calls -- the CARRIED ROW.  A call sweeps the new events (a chunk) of its
// slots below it, reports the window scan of the new last row and leaves that row in the carried row's place.
//
//   * one wave-task = (group of slots, contig, strand), all columns in one sweep.  The lane layout is a base class shape of
//     the fill (kClassShapes), chosen by the CHUNK length; 64 / L slots share a wave; chunks of different lengths share a
//     wave when they agree modulo R and are laid out from the end (MixedQuad): lane and register of the last row are the
//     wave's, a shorter chunk begins in a later lane g0.
//   * the step is strip_step: FIRST = true for a slot's first chunk (constant boundary 0, a path starts in its own column:
//     exactly the fill's sweep), FIRST = false below a carried row -- lane g0 takes `up` (and its start column) from the
//     carried row at its column, its diagonal is the previous step's `up`.  The host never mixes the two kinds in a wave.
//     Column 0 needs no special case: there is no column -1 (the diagonal input is +inf) and its `up` carries start 0.
//   * the carried row is loaded four columns per 16-byte access, one block of four steps ahead, like the reference levels;
//     the new last row (lane lq, register rq) is collected four columns at a time and stored with ordinary vector stores IN
//     PLACE: column j is read for step j + g0 at the latest and written at step j + lq >= j + g0 by the same wave, memory
//     operations of a wave are issued in order, and no other wave touches the row of this (slot, contig, strand).
//   * rows of all (slot, job) pairs lie back to back, total_columns per slot and no padding in between (sfa_session_bytes is
//     exactly rows x columns); the block loads of a sweep over-run its row by up to 70 columns on both sides.  What they find
//     there -- another row, maybe while its wave rewrites it, or the pads around the allocation -- is a cost (never a NaN:
//     slots with non-finite events are not swept) and only reaches cells of columns < 0, which are forced to +inf, or
//     >= rlen, whose reference level is the +inf padding and which nothing of a column < rlen depends on.
//   * the window scan of the new last row (src/sigfish.c:891-901) uses windows of the slot's TOTAL length, not the chunk's;
//     every window's first strict minimum, its column and (TRACK) its start column are kept, the top-2 per (slot, job) goes
//     to HBM and sdtw_session_rows_kernel merges the jobs in processing order and writes the rows.
// All arithmetic is the fill's: every cell is the same pure fp32 function of its three neighbours, so rows equal those of
// sfa_align_batch over the concatenated events bit for bit.
#pragma once

#include "sdtw_strips.hpp"
#include "session_plan.hpp"  // SessionClass, kSessionMaxClasses: the class table is the host planner's

namespace sfa {

constexpr int kSessionPad = 256;       // words in front of and behind the carried rows of a session (over-run of the block loads)

// Everything a launch reads.  "Entry" k: a slot's piece of this launch (a chunk of up to 2048 events, or a piece of a longer one).
struct SessionArgs {
    const float *events;      // the call's events, concatenated
    const int32_t *w_entry;   // [n_groups * 4] entry per (group, wave slot) or -1
    const int32_t *g_qlen;    // [n_groups] longest piece of the group
    const int32_t *k_call;    // [n_entries] index of the slot in the call (bad flag, partial results)
    const int32_t *k_slot;    // [n_entries] slot of the session
    const int64_t *k_off;     // [n_entries] first event of the piece in `events`
    const int32_t *k_len;     // [n_entries] events of the piece
    const int32_t *k_total;   // [n_entries] events of the slot up to and including the piece: the window length
    const uint8_t *bad;       // [n_call] the slot's chunk holds a NaN / inf (sdtw_screen_kernel): not swept
    const float *ref;         // as DpArgs
    const int64_t *job_off;
    const int32_t *job_len;
    const int64_t *col_off;   // [n_jobs] first column of job j inside a slot's carried row
    float *row_c;             // carried costs [n_slots][row_stride], kSessionPad words in front
    int32_t *row_s;           // carried start columns, same layout (TRACK)
    int64_t row_stride;       // total_columns
    float *p_best, *p_second; // [n_call][n_jobs] top-2 of the windows of the new last row
    int32_t *p_end, *p_st;    // column of the best window's first strict minimum, start column of the path into it
    SessionClass cls[kSessionMaxClasses];
    int32_t n_cls, n_jobs, n_tasks;
    int32_t *p_top5;          // [n_call][n_jobs][kTop5Words] SEC: the candidate list of the new last row's windows (behind all else: the
                              // kernels without SEC read the layout they always have)
};

template <typename T>
struct __attribute__((packed, aligned(4))) Quad4 {
    T v[4];
};

// last row of the lane's R rows: register rq (wave-uniform)
template <int R, bool TRACK, typename CF, typename CI>
__device__ __forceinline__ void session_last_row(const CF &c, const CI &s, const int rq, float &cl, int &sl) {
    if constexpr (R >= 32) {
        pick_row<R>(c, s, rq, cl, sl);
    } else {
        cl = c[rq];
        sl = TRACK ? static_cast<int>(s[rq]) : 0;
    }
}

// SEC: the sorted list of the 5 best windows (top5_offer, row_rules.hpp: update_aln's rule) per (wave, wave slot) in LDS, as lds_t5 of
// sdtw_sec_fill_kernel -- the tracked kernel has no VGPRs to spare.  An entry is (score bits, column of the window's first strict
// minimum, start column of the path into it; -1 without TRACK): the job is the task's own.  Only the owner lane touches its list,
// once per window; Top2 and what it writes are as without SEC.
template <int R, int L, bool TRACK, bool FIRST, bool SEC = false>
__device__ __forceinline__ void session_body(const SessionArgs &a, const SessionClass cd, const int task_local, float *lds_f, int *lds_i,
                                             int *lds_t5 = nullptr) {
    constexpr int NS = 64 / L;
    const int job = task_local / cd.n_groups;  // job-major: neighbouring waves stream the same reference
    const int group = cd.group_base + (task_local - job * cd.n_groups);
    const int lane = threadIdx.x & 63;
    const int g = lane & (L - 1);
    const int ws = lane / L;

    const int qlen = __builtin_amdgcn_readfirstlane(a.g_qlen[group]);
    const int lq = (qlen - 1) / R;  // lane / register of everybody's last row
    const int rq = (qlen - 1) - lq * R;
    const int t_begin = sweep_begin(lq);
    const int k = a.w_entry[group * 4 + ws];
    const int call = k >= 0 ? a.k_call[k] : 0;
    const bool live = k >= 0 && !a.bad[call];
    const int myq = live ? a.k_len[k] : qlen;
    const int g0 = (qlen - myq) / R;  // (lengths of a group agree modulo R)
    const bool lane0 = g == g0;
    const int total = live ? a.k_total[k] : qlen;  // window length of the last-row scan
    const int64_t slot = live ? a.k_slot[k] : 0;   // (a wave slot without work reads slot 0's row and writes nothing)
    const bool owner = live && g == lq;

    float x[R];
    {
        const float *q = a.events + (live ? a.k_off[k] : 0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = (g - g0) * R + r;
            x[r] = (live && i >= 0 && i < myq) ? q[i] : 0.0f;
        }
    }
    Exchange xc;
    xc.init(lds_f, lds_i, threadIdx.x >> 6, ws, g, L, g0);
    xc.template set_boundary<TRACK>(lane0, 0.0f);

    const int rlen = a.job_len[job];
    const float *yp = a.ref + a.job_off[job] - g + t_begin;  // this lane's column at step t is t - g
    const int64_t row0 = kSessionPad + slot * a.row_stride + a.col_off[job];
    float *crow = a.row_c + row0;
    int32_t *srow = TRACK ? a.row_s + row0 : nullptr;
    const float *cin = crow + (t_begin - g0);  // lane g0's column at step t is t - g0
    const int32_t *sin = TRACK ? srow + (t_begin - g0) : nullptr;

    typename Vec<float, R>::type c;
    typename Vec<int, R>::type s;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        c[r] = INFINITY;
        s[r] = 0;
    }
    float dprev = INFINITY;
    int sdprev = 0;

    Top2 top;
    top.init();
    int top_st = -1;
    int *t5 = nullptr;
    if constexpr (SEC) {
        t5 = lds_t5 + ((threadIdx.x >> 6) * 4 + ws) * kTop5Words;
        if (owner) top5_init(t5);  // (an empty entry: column -1)
    }
    float wmin = INFINITY;
    int wpos = -1, wst = -1;
    int wend = min(total, rlen);  // end of this slot's current window
    auto next_end = [&]() {
        int n = __builtin_amdgcn_readlane(wend, 0);
#pragma unroll
        for (int sl = 1; sl < NS; ++sl) n = min(n, __builtin_amdgcn_readlane(wend, sl * L));
        return n;
    };
    int nxt = next_end();  // wave-uniform: the column behind which the next window of any slot ends

    typedef Quad4<float> F4;
    typedef Quad4<int32_t> I4;
    F4 ycur = *reinterpret_cast<const F4 *>(yp);
    F4 bcur = {{0.0f, 0.0f, 0.0f, 0.0f}};
    I4 scur = {{0, 0, 0, 0}};
    if (!FIRST) {
        bcur = *reinterpret_cast<const F4 *>(cin);
        if (TRACK) scur = *reinterpret_cast<const I4 *>(sin);
    }
    int e = 0;  // steps executed; the next step is t = t_begin + e
    // ---- prologue: the last row has not reached column 0.  Lane g0 may still be in front of column 0: there is no carried
    // value there, the boundary is +inf (as the cells of those columns are) ----
    const int e_main = lq - t_begin;
    for (; e < e_main; e += 4) {
        const F4 ynext = *reinterpret_cast<const F4 *>(yp + e + 4);
        F4 bnext = bcur;
        I4 snext = scur;
        if (!FIRST) {
            bnext = *reinterpret_cast<const F4 *>(cin + e + 4);
            if (TRACK) snext = *reinterpret_cast<const I4 *>(sin + e + 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col0 = t_begin + e + u - g0;  // column of the lane that holds the chunk's first row
            const float bup = col0 >= 0 ? bcur.v[u] : INFINITY;
            strip_step<false, FIRST, TRACK, R>(c, s, dprev, sdprev, x, ycur.v[u], col0, lane0, xc, bup, scur.v[u]);
        }
        ycur = ynext;
        bcur = bnext;
        scur = snext;
    }
    // ---- main: block b covers last-row columns 4b .. 4b + 3 ----
    for (int cb = 0; cb < rlen; cb += 4, e += 4) {
        const F4 ynext = *reinterpret_cast<const F4 *>(yp + e + 4);
        F4 bnext = bcur;
        I4 snext = scur;
        if (!FIRST) {
            bnext = *reinterpret_cast<const F4 *>(cin + e + 4);
            if (TRACK) snext = *reinterpret_cast<const I4 *>(sin + e + 4);
        }
        F4 oc;
        I4 os;
        const bool edge = cb + 4 > rlen;  // wave-uniform: the last block of a row whose length is no multiple of four
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col0 = t_begin + e + u - g0;
            strip_step<false, FIRST, TRACK, R>(c, s, dprev, sdprev, x, ycur.v[u], col0, lane0, xc, bcur.v[u], scur.v[u]);
            const int col = cb + u;  // of the last row
            float cl;
            int sl;
            session_last_row<R, TRACK>(c, s, rq, cl, sl);
            oc.v[u] = cl;
            os.v[u] = sl;
            if (edge && col >= rlen) continue;  // (wave-uniform)
            const bool lt = cl < wmin;  // first strict minimum of the window (src/sigfish.c:892-899)
            wmin = lt ? cl : wmin;
            wpos = lt ? col : wpos;
            if (TRACK) wst = lt ? sl : wst;
            if (__builtin_expect(col + 1 == nxt, 0)) {  // a window of some slot ends behind this column
                const bool ending = wend == col + 1;
                const bool became_best = top.offer_if(ending, wmin, wpos, job);
                top_st = became_best ? wst : top_st;
                if constexpr (SEC) {
                    if (ending && owner) top5_offer(t5, wmin, wpos, TRACK ? wst : -1);
                }
                wmin = ending ? INFINITY : wmin;
                wpos = ending ? -1 : wpos;
                wst = ending ? -1 : wst;
                wend = ending ? wend + min(total, rlen - wend) : wend;
                nxt = next_end();
            }
        }
        if (owner) {  // the new last row takes the carried row's place
            if (!edge) {
                *reinterpret_cast<F4 *>(crow + cb) = oc;
                if (TRACK) *reinterpret_cast<I4 *>(srow + cb) = os;
            } else {
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    if (cb + u < rlen) {
                        crow[cb + u] = oc.v[u];
                        if (TRACK) srow[cb + u] = os.v[u];
                    }
                }
            }
        }
        ycur = ynext;
        bcur = bnext;
        scur = snext;
    }
    if (owner) {
        const int64_t o = static_cast<int64_t>(call) * a.n_jobs + job;
        a.p_best[o] = top.best;
        a.p_second[o] = top.second;
        a.p_end[o] = top.end;
        a.p_st[o] = top_st;
        if constexpr (SEC) {  // (a chunk of several pieces: the last launch's list stays)
            for (int w = 0; w < kTop5Words; ++w) a.p_top5[o * kTop5Words + w] = t5[w];
        }
    }
}

// grid: ceil(n_tasks / 4) blocks of 256 threads, one task per wave.  TRACK: start columns are carried and propagated
// (strip_step's tracking branch); else costs only (SFA_SESSION_NO_START).  SEC: the windows' candidate lists as well
// (sfa_session_candidates_config); sessions that do not ask for them launch the kernels without.
template <bool TRACK, bool SEC = false>
__global__ void __launch_bounds__(256, TRACK ? 2 : 3) sdtw_session_kernel(const SessionArgs a) {
    const int task = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    __shared__ float lds_f[4 * kXchWordsPerWave];
    __shared__ int lds_i[TRACK ? 4 * kXchWordsPerWave : 1];
    int *lds_t5 = nullptr;
    if constexpr (SEC) {
        __shared__ int t5[4 * 4 * kTop5Words];
        lds_t5 = t5;
    }
    if (task >= a.n_tasks) return;  // wave-uniform
    int ci = 0;
    while (ci + 1 < a.n_cls && task >= a.cls[ci + 1].task_base) ++ci;
    const SessionClass cd = a.cls[ci];
    const int tl = task - cd.task_base;
#define SFA_SHAPE(RR, LL)                                                     \
    case (RR) * 256 + (LL):                                                   \
        if (cd.first)                                                         \
            session_body<RR, LL, TRACK, true, SEC>(a, cd, tl, lds_f, lds_i, lds_t5);  \
        else                                                                  \
            session_body<RR, LL, TRACK, false, SEC>(a, cd, tl, lds_f, lds_i, lds_t5); \
        break;
    switch (cd.R * 256 + cd.lanes) {
        SFA_SHAPE(32, 64) SFA_SHAPE(32, 32) SFA_SHAPE(32, 16)
        SFA_SHAPE(16, 16) SFA_SHAPE(8, 16) SFA_SHAPE(4, 16)
        default:
            break;
    }
#undef SFA_SHAPE
}

// instantiated in sdtw_inst_session_track.hip / sdtw_inst_session_cost.hip, with SEC in sdtw_inst_session_track_sec.hip /
// sdtw_inst_session_cost_sec.hip
extern template __global__ void sdtw_session_kernel<true>(const SessionArgs);
extern template __global__ void sdtw_session_kernel<false>(const SessionArgs);
extern template __global__ void sdtw_session_kernel<true, true>(const SessionArgs);
extern template __global__ void sdtw_session_kernel<false, true>(const SessionArgs);

struct SessionRowsArgs {
    const int32_t *call_slot;  // [n_call] slot of the session, -1: no row to write (no new events, or the slot is poisoned)
    const uint8_t *bad;        // [n_call]
    const float *p_best, *p_second;
    const int32_t *p_end, *p_st;
    RefTables ref;
    ResultRow *rows;           // [n_slots] the current row of every slot
    int32_t n_call, n_jobs;
    int32_t track;             // 0: SFA_SESSION_NO_START -- the coordinate that needs the start column is -1
};

struct SessionCandArgs {
    const int32_t *call_slot;  // as SessionRowsArgs
    const uint8_t *bad;
    const int32_t *p_top5;     // SessionArgs::p_top5
    RefTables ref;
    ResultRow *cand;           // [n_slots][4] the candidates behind every slot's current row, best first
    int32_t n_call, n_jobs;
    int32_t n_cand;            // ranks asked for (1..4): rows of the ranks behind are valid = 0
    int32_t track;             // as SessionRowsArgs
};

// sfa_session_keep_events: an event-mode session that keeps its slots' events for sfa_session_event_maps
struct SessionKeepArgs {
    const float *events;      // the call's events as staged for the sweep, concatenated
    const int64_t *ch_off;    // [n + 1] first event of every entry of the call
    const int32_t *slot;      // [n] slot of the session
    const int32_t *have;      // [n] events the slot held before the call
    float *keep;              // [n_slots][max_events] the slots' events since their last reset
    uint8_t *over;            // [n_slots] 1: the slot has received more than max_events events (its kept events are the first max_events)
    int32_t n, max_events;
};

#ifdef SFA_DEFINE_SESSION_KERNELS  // plain kernels: defined in exactly one translation unit (sfa_session.hip)
// Appends every entry's events to its slot's kept events, d_keep[slot][have, have + len), clipped at max_events; a slot's first
// chunk after a reset clears its overflow flag, a clipped one sets it.  One block per entry; consecutive lanes copy
// consecutive words.  The host has checked the slots' range and names a slot once per call.
__global__ void __launch_bounds__(256) sdtw_session_keep_kernel(const SessionKeepArgs a) {
    const int i = blockIdx.x;
    if (i >= a.n) return;
    const int64_t off = a.ch_off[i];
    const int64_t len = a.ch_off[i + 1] - off;
    const int have = a.have[i];
    const int64_t slot = a.slot[i];
    const int64_t room = have < a.max_events ? a.max_events - have : 0;
    const int take = static_cast<int>(len < room ? len : room);
    const float *src = a.events + off;
    float *dst = a.keep + slot * a.max_events + have;
    for (int j = threadIdx.x; j < take; j += 256) dst[j] = src[j];
    if (threadIdx.x == 0 && (have == 0 || len > room)) a.over[slot] = len > room ? 1 : 0;
}

// the jobs' partial top-2 of every slot of the call merged in processing order (a later job wins ties), then contig, strand,
// mapq, flip and offset (src/sigfish.c:969-983): what sdtw_finalize_kernel does for a batch
__global__ void __launch_bounds__(64) sdtw_session_rows_kernel(const SessionRowsArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_call) return;
    const int slot = a.call_slot[i];
    if (slot < 0 || a.bad[i]) return;
    struct Win {
        int end, st, job;
    };
    Top2Merge<Win> m({-1, -1, -1});
    for (int j = 0; j < a.n_jobs; ++j) {
        const int64_t o = static_cast<int64_t>(i) * a.n_jobs + j;
        m.offer(a.p_best[o], a.p_second[o], {a.p_end[o], a.p_st[o], j});
    }
    ResultRow r = primary_row(m.best, m.second, m.pay.job, a.ref);
    if (m.pay.job >= 0) {
        place_row(r, m.pay.st, m.pay.end, a.ref);
        if (!a.track) drop_start(r);
    }
    a.rows[slot] = r;
}

// Session candidates: the jobs' lists of every slot of the call merged in processing order, each list worst entry first (the
// order of sdtw_sec_finalize_kernel over chunks), and the four candidates behind the winner written as rows, best first: the
// layout of sfa_secondary_rows.  Slots the rows kernel skips keep their stored candidates.  One lane per slot of the call.
__global__ void __launch_bounds__(64) sdtw_session_cand_kernel(const SessionCandArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_call) return;
    const int slot = a.call_slot[i];
    if (slot < 0 || a.bad[i]) return;
    Top5<1> t;  // the payload is job * 5 + entry: where the candidate's columns are
    const int32_t *lists = a.p_top5 + static_cast<int64_t>(i) * a.n_jobs * kTop5Words;
    for (int j = 0; j < a.n_jobs; ++j)
        for (int e = 0; e < 5; ++e) {
            const int32_t *w = lists + j * kTop5Words + 3 * e;
            if (w[1] >= 0) t.offer(row_float(w[0]), j * 5 + e);
        }
    SFA_ROW_UNROLL
    for (int k = 1; k < 5; ++k) {
        ResultRow r = no_row();
        int x;
        const float score = t.rank(k, x);
        if (k <= a.n_cand && x >= 0) {
            const int job = x / 5;
            const int32_t *w = lists + job * kTop5Words + 3 * (x - job * 5);  // (score bits, end, start)
            r = secondary_row(score, t.score(k + 1), job, w[2], w[1], a.ref);
            if (!a.track) drop_start(r);
        }
        a.cand[static_cast<int64_t>(slot) * 4 + (k - 1)] = r;
    }
}
#endif

}  // namespace sfa
