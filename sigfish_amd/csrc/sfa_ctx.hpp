// sfa_ctx.hpp -- what the units of the C-ABI share (include/sigfish_amd.h): error reporting, the buffer, stream and event types
// that free themselves (sfa_buf.hpp: Buf<Mem>; here its two allocators, DevBuf / PinBuf), the context, and the few internal
// functions that cross unit boundaries.  The context (sfa_ctx) is its streams and events, the options, and one struct per stage
// (namespace ctx) holding that stage's buffers, what it keeps between calls and reserve(), the sizes of its buffers; sfa_destroy
// names none of them.
//   sfa_context.hip  contexts: init / destroy, devices, options, profile, small utilities
//   sfa_align.hip    the alignment stage: planner -> launches (wave kernels, row strips) -> rows; the batch entry points
//   sfa_maps.hip     event maps of the last call's rows, and the core sfa_session_event_maps shares with it (sdtw_path.hpp)
//   sfa_session.hip  alignment sessions: a slot's sweep extended chunk by chunk below its carried row (sdtw_session.hpp)
//                    -- its state one struct per feature (namespace sess, sfa_session_state.hpp), its host rules in session_plan.hpp
//                    (pure C++, as sfa_plan.hpp); on a group context a session spread over the shards (session_spread.hpp)
//   sfa_session_targets.hip  what a session knows about the reference beside its rows -- targets, groups, caps, reach lists --
//                    and the query calls that read a slot's carried row with it (session_query.hpp: which entries launch)
//   sfa_pre.hip      the stages in front of it on the device: raw samples / BLOW5 records in (events_kernels.hpp, blow5_kernels.hpp)
// There is NO CPU fallback: every failure is reported through the return code + sfa_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sigfish_amd.h"
#include "sdtw_kernels.hpp"  // BatchStatus, the sizes of the kernels' records
#include "sfa_buf.hpp"
#include "sfa_plan.hpp"

namespace {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    sfa::last_error_slot() = buf;
    return code;
}


#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(SFA_ENODEV, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                  \
    } while (0)

// after a kernel launch: a rejected launch (bad configuration, missing code object) is SFA_EKERNEL
#define KERNEL_TRY()                                                                                            \
    do {                                                                                                        \
        hipError_t e_ = hipGetLastError();                                                                      \
        if (e_ != hipSuccess) return fail(SFA_EKERNEL, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// The context's buffers (sfa_buf.hpp): device memory and page-locked host memory
struct DevMem {
    static constexpr const char *name = "hipMalloc";
    static void *alloc(size_t bytes) {
        void *p = nullptr;
        return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
    }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinMem {
    static constexpr const char *name = "hipHostMalloc";
    static void *alloc(size_t bytes) {
        void *p = nullptr;
        return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    static void free(void *p) { (void)hipHostFree(p); }
};
using DevBuf = sfa::Buf<DevMem>;
using PinBuf = sfa::Buf<PinMem>;

// reserve(bytes) of every (buffer, bytes) pair in turn; the first failure ends it and is the result
template <class B, class... Rest>
int reserve_all(B &buf, size_t bytes, Rest &&...rest) {
    if (int rc = buf.reserve(bytes)) return rc;
    if constexpr (sizeof...(rest) > 0) return reserve_all(rest...);
    return SFA_OK;
}

// A stream / an event of the context: created by create_context (sfa_context.hip), destroyed with the context
template <class T, hipError_t (*Destroy)(T)>
struct Owned {
    T h = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    ~Owned() {
        if (h) (void)Destroy(h);
    }
    operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// One host thread per shard of a group context (sfa_init_devices), alive as long as the context: HIP's current device and
// sfa_last_error are per thread, so every shard's calls are made from its own thread -- but not from a fresh one per call
// (round 2: std::async per shard and call, i.e. a thread creation + the runtime's per-thread set-up inside every batch).
class ShardWorker {
  public:
    ShardWorker() : th_([this] { loop(); }) {}
    ~ShardWorker() {
        {
            std::lock_guard<std::mutex> lk(m_);
            quit_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void post(std::function<int()> job) {
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = std::move(job);
            state_ = 1;
        }
        cv_.notify_all();
    }
    std::pair<int, std::string> wait() {  // of the job posted last
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return state_ == 2; });
        state_ = 0;
        return {rc_, err_};
    }

  private:
    void loop() {
        for (;;) {
            std::function<int()> job;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return quit_ || state_ == 1; });
                if (quit_) return;
                job = std::move(job_);
            }
            const int rc = job();
            {
                std::lock_guard<std::mutex> lk(m_);
                rc_ = rc;
                err_ = rc ? sfa::last_error_slot() : std::string();
                state_ = 2;
            }
            cv_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::function<int()> job_;
    int state_ = 0;  // 0 idle, 1 posted, 2 done
    bool quit_ = false;
    int rc_ = 0;
    std::string err_;
    std::thread th_;  // last: started when everything else exists
};

}  // namespace

namespace sfa {
struct EvArgs;    // events_kernels.hpp: argument blocks of the event detection and of the automatic query start, which
struct AutoArgs;  // ctx::RawSignal fills from its buffers (defined in sfa_pre.hip, the one unit that launches those kernels)

// the kernels' row (row_rules.hpp) is the C-ABI's, field for field
#define SFA_SAME_FIELD(f) (offsetof(ResultRow, f) == offsetof(sfa_result_t, f) && sizeof(ResultRow::f) == sizeof(sfa_result_t::f))
static_assert(sizeof(ResultRow) == sizeof(sfa_result_t) && SFA_SAME_FIELD(rid) && SFA_SAME_FIELD(pos_st) && SFA_SAME_FIELD(pos_end) && SFA_SAME_FIELD(score) &&
                  SFA_SAME_FIELD(score2) && SFA_SAME_FIELD(strand) && SFA_SAME_FIELD(mapq) && SFA_SAME_FIELD(valid) && SFA_SAME_FIELD(pad),
              "result row layout");
#undef SFA_SAME_FIELD
inline sfa_result_t to_result(const ResultRow &r) {
    sfa_result_t o;
    memcpy(&o, &r, sizeof o);
    return o;
}
}  // namespace sfa

// ---- the context's state, one struct per stage that owns it: its buffers, what it keeps between calls, and reserve(), the one
// place that says how large each buffer has to be.  Every buffer frees itself with the context. ----
namespace ctx {

struct RefModel {  // the reference event model (immutable after init)
    int32_t num_ref = 0, n_jobs = 0;
    int64_t total_cols = 0;  // sum over jobs of rlen
    std::vector<int32_t> h_job_len;
    std::vector<int64_t> h_job_off;   // [n_jobs] column 0 of every (contig,strand) array in d_ref
    std::vector<int32_t> h_ref_off;   // [num_ref] ref_st_offset
    DevBuf d_ref, d_job_off, d_job_len, d_job_contig, d_job_strand, d_ref_len, d_ref_off;
    int reserve(size_t ref_bytes) {
        const size_t j = n_jobs, r = num_ref;
        return reserve_all(d_ref, ref_bytes, d_job_off, sizeof(int64_t) * j, d_job_len, sizeof(int32_t) * j, d_job_contig, sizeof(int32_t) * j,
                           d_job_strand, j, d_ref_len, sizeof(int32_t) * r, d_ref_off, sizeof(int32_t) * r);
    }
    // what the finalize kernels read of the model (row_rules.hpp)
    sfa::RefTables tables() const { return {d_job_contig.as<int32_t>(), d_job_strand.as<int8_t>(), d_ref_len.as<int32_t>(), d_ref_off.as<int32_t>()}; }
};

struct CallerIO {  // queries in, rows out, of the entry points that take host memory
    DevBuf d_queries, d_out;
    PinBuf h_out, h_small;
    PinBuf h_queries;  // sfa_align_events: the gathered event means (page-locked: the upload from here is asynchronous)
    int32_t pending_n = -1;  // reads of the batch submitted with sfa_submit_batch and not yet collected
    int reserve(int64_t query_floats, size_t n) {
        return reserve_all(d_queries, sizeof(float) * static_cast<size_t>(std::max<int64_t>(query_floats, 1)), d_out, sizeof(sfa_result_t) * n,
                           h_out, sizeof(sfa_result_t) * n);
    }
};

struct Status {  // what a batch reports about itself
    DevBuf d_bad;    // sdtw_screen_kernel: per-read flag
    DevBuf d_block;  // the batch's sfa::BatchStatus (sdtw_kernels.hpp) ...
    PinBuf h_block;  // ... and where it is copied once the batch is through (resolve_profile reads it)
    int reserve(size_t n) { return reserve_all(d_bad, n, d_block, sizeof(sfa::BatchStatus), h_block, sizeof(sfa::BatchStatus)); }
    sfa::BatchStatus *dev() const { return d_block.as<sfa::BatchStatus>(); }
    const sfa::BatchStatus *host() const { return h_block.as<sfa::BatchStatus>(); }  // nullptr: no batch yet
};

struct WaveKernels {  // every route: the plan in the staging area, partial results of the fill tasks, the winners
    DevBuf d_stage, d_pbest, d_pend, d_pjob, d_psecond, d_wjob, d_wend, d_wscore, d_tst, d_ck;
    DevBuf d_wchunk;   // winning chunk of every read
    DevBuf d_started;  // counter of the fill's tasks that have begun (IssuePriority)
    PinBuf h_stage;
    sfa::BatchPlan plan;  // plan of the batch being submitted (scratch included)
    int32_t span_sixteenths = 0;  // pass 2's head start on the HBM-snapshot route follows the spans of the previous batch's alignments: sixteenths of the query length (0: not known yet -> a whole query length)
    int64_t quad_limit_ms = 0;    // the limit the last batch's waits actually ran with (floor applied), for the error message
    // n_part: partial results, four per (quad, chunk)
    int reserve(size_t stage_bytes, size_t n_part, size_t n, int64_t ck_floats) {
        if (int rc = reserve_all(h_stage, stage_bytes, d_stage, stage_bytes, d_pbest, 4 * n_part, d_pend, 4 * n_part, d_pjob, 4 * n_part,
                                 d_psecond, 4 * n_part, d_wjob, 4 * n, d_wend, 4 * n, d_tst, 8 * n, d_wscore, 4 * n, d_wchunk, 4 * n, d_started, 64))
            return rc;
        return ck_floats > 0 ? d_ck.reserve(sizeof(float) * ck_floats) : SFA_OK;
    }
};

struct FusedLaunch {  // the kernel's argument block in device memory (DpArgs::self), ticket counter, completed fill tasks per quad
    DevBuf d_args, d_ticket, d_quaddone;
    int reserve(size_t n_quads) { return reserve_all(d_args, sizeof(sfa::DpArgs), d_ticket, 64, d_quaddone, 4 * n_quads); }
};

struct LdsRoute {  // LDS-checkpoint fill: records of the best windows, their step, per-read best score
    DevBuf d_bestrec, d_beste, d_gbest;
    int reserve(size_t n_part, size_t n) {
        return reserve_all(d_bestrec, sizeof(float) * sfa::kLdsCkPlanes * 64 * n_part / 4, d_beste, 4 * n_part, d_gbest, 4 * n);
    }
};

struct Segments {  // column segments: the states at the hand-overs, one verdict per quad
    DevBuf d_verify, d_segfail;
    PinBuf h_flags;
    int64_t seg_reruns = 0;         // batches walked again because a segment hand-over did not verify
    bool no_segments_once = false;  // re-run of a batch whose segment hand-overs did not verify
    int reserve(const sfa::BatchPlan &p, size_t n_jobs) {
        const size_t q = p.n_quads;
        return reserve_all(d_verify, sizeof(float) * 64 * (p.max_R + 1) * 2 * static_cast<size_t>(p.n_seg) * n_jobs * q, d_segfail, 4 * q, h_flags, 4 * q);
    }
};

struct Strips {  // row strips (queries beyond SFA_MAX_QUERY, sdtw_strips.hpp)
    DevBuf d_lprog, d_lticket;  // pipelined strips: progress counters, ticket
    DevBuf d_bndc, d_long, d_lbest, d_lsecond, d_lend, d_lwin, d_lck;
    PinBuf h_long;
    bool long_pending = false;
    int64_t strip_limit_ms = 0;  // the limit the last batch's waits actually ran with (floor applied), for the error message
    int reserve_staging(size_t bytes) { return reserve_all(h_long, bytes, d_long, bytes); }
    // n_part: (read, job) pairs; a freshly grown d_bndc is set to 3.4e38 everywhere on `st` (see the pad note in sdtw_strips.hpp)
    int reserve(size_t prog_bytes, size_t bndc_floats, size_t lck_floats, size_t n_part, size_t n_long, hipStream_t st) {
        const size_t bndc_cap = d_bndc.cap;
        if (int rc = reserve_all(d_lprog, prog_bytes, d_lticket, 128, d_bndc, sizeof(float) * bndc_floats, d_lbest, 4 * n_part, d_lsecond, 4 * n_part,
                                 d_lend, 4 * n_part, d_lwin, 4 * 5 * n_long, d_lck, sizeof(float) * lck_floats))
            return rc;
        if (d_bndc.cap != bndc_cap) HIP_TRY(hipMemsetAsync(d_bndc.p, 0x7f, d_bndc.cap, st));
        return SFA_OK;
    }
    // secondary mappings of the long reads ("secondary_strips"): the candidate lists of pass 1, the ranks of the merge with their
    // traced columns; sizes in words, from sfa::LongPlan
    DevBuf d_lp5, d_lranks;
    int reserve_secondary(size_t list_words, size_t rank_words) { return reserve_all(d_lp5, 4 * list_words, d_lranks, 4 * rank_words); }
};

struct Secondaries {  // secondary mappings: top-5 partials, merged candidates, their traced columns, rows [n][4]
    DevBuf d_p5, d_swin, d_sts, d_sec;
    int32_t sec_n = -1;  // reads of the last call whose secondaries d_sec holds
    int reserve(size_t n_part, size_t n) { return reserve_all(d_p5, 4 * sfa::kTop5Words * n_part, d_swin, 4 * 15 * n, d_sts, 4 * 10 * n); }
    int reserve_rows(size_t n) { return d_sec.reserve(4 * sizeof(sfa::ResultRow) * n); }  // (only a call that keeps its own rows)
};

struct RawSignal {  // sfa_align_raw: samples, prefix sums, t-statistics, events, query windows, raw-coordinate columns
    DevBuf e_raw, e_rawoff, e_scale, e_sum, e_sumsq, e_t1, e_t2, e_evoff, e_evstart, e_evlen, e_evmean, e_evstdv, e_nev, e_qstart,
        e_qoff, e_b0, e_b1, e_b2, e_flag, e_qev, e_pflag;
    bool eev_pending = false;
    sfa::EvArgs detector_args(int32_t n) const;  // every buffer of the detection; the caller adds parameters and routes
    sfa::AutoArgs auto_args(int32_t n) const;    // the automatic start reuses e_sumsq / e_t1 and writes behind the counts in e_nev
    int reserve_samples(int64_t total, size_t n) { return reserve_all(e_raw, 2 * static_cast<size_t>(std::max<int64_t>(total, 1)), e_rawoff, 8 * (n + 1)); }
    int reserve(int64_t total, size_t n, size_t ev_total) {
        const size_t t1 = static_cast<size_t>(std::max<int64_t>(total, 1));
        if (int rc = reserve_samples(total, n)) return rc;
        return reserve_all(e_scale, 8 * n, e_sum, 8 * (total + n), e_sumsq, 8 * (total + n), e_t1, 4 * t1, e_t2, 4 * t1, e_evoff, 8 * (n + 1),
                           e_evstart, 4 * ev_total, e_evlen, 4 * ev_total, e_evmean, 4 * ev_total, e_evstdv, 4 * ev_total, e_nev, 8 * n,
                           e_qstart, 8 * n, e_qoff, 8 * (n + 1), e_flag, 4 * n, e_pflag, 4 * n, e_b0, 4 * n, e_b1, 4 * n, e_b2, 4 * n);
    }
};

struct Blow5 {  // sfa_align_blow5: record bytes, inflated payloads, field rows
    DevBuf b_in, b_inoff, b_out, b_outoff, b_len, b_head, b_bad;
    DevBuf b_zscratch, b_zoff;  // zstd records: every decoder's tables and literals (zstd_kernels.hpp), and where they start
    PinBuf h_head;
    bool bev_pending = false;
    int64_t blow5_fallbacks = 0;  // batches handed to the host reader because the device declined a record
    // the decompressor's own buffers; out_bytes < 0: records that are not compressed; scratch_bytes > 0: zstd records
    int reserve_inflate(size_t in_bytes, int64_t out_bytes, size_t n, int64_t scratch_bytes = 0) {
        if (int rc = reserve_all(b_in, in_bytes + 128, b_inoff, 8 * (n + 1), b_len, 4 * n)) return rc;
        if (scratch_bytes > 0)
            if (int rc = reserve_all(b_zscratch, static_cast<size_t>(scratch_bytes) + 64, b_zoff, 8 * (n + 1))) return rc;
        return out_bytes < 0 ? SFA_OK : reserve_all(b_out, static_cast<size_t>(out_bytes) + 64, b_outoff, 8 * (n + 1));
    }
    int reserve(size_t in_bytes, int64_t out_bytes, size_t n, size_t head_bytes, int64_t scratch_bytes = 0) {
        if (int rc = reserve_inflate(in_bytes, out_bytes, n, scratch_bytes)) return rc;
        return reserve_all(b_head, n * head_bytes, h_head, n * head_bytes + 8 * n, b_bad, 4 * n);
    }
};

// The scratch of one event-maps call (sdtw_path.hpp): packed moves of a slice of rows, its row descriptors (the query offsets
// behind them), its maps, where every walk ended.  A context has one for sfa_event_maps, every session its own for
// sfa_session_event_maps: neither call disturbs the other's.
struct MapScratch {
    DevBuf d_mv, d_prow, d_pairs, d_pfirst;
    PinBuf h_pairs;
    int reserve(size_t mv_bytes, size_t prow_bytes, size_t n_rows, size_t out_pairs) {
        return reserve_all(d_mv, mv_bytes, d_prow, prow_bytes, d_pairs, 8 * out_pairs, d_pfirst, 4 * n_rows, h_pairs, 8 * out_pairs + 4 * n_rows);
    }
};

// sfa_event_maps: what the last align call left behind -- its read count (-1: none), the offsets of its queries and where they
// are (the context's d_queries, or the caller's memory after sfa_align_batch_device); a group context keeps the count
struct EventMaps : MapScratch {
    int32_t map_n = -1;
    std::vector<int64_t> map_q_off;
    const float *map_queries = nullptr;
};

struct TaskTimes {  // -DSFA_TASK_TIMES builds
    DevBuf d_times;   // start / end / SIMD position of every wave-task of the last fill
    int64_t n_times = 0;
    DevBuf d_ltimes;  // ... and of the last pipelined pass 1 over row strips (tools/strip_task_times.py)
    int64_t n_ltimes = 0;
};

}  // namespace ctx

struct sfa_ctx {
    // A GROUP context (sfa_init_devices) owns one ordinary context per listed device and nothing else: every batch is cut
    // into contiguous read ranges, one per shard, which run concurrently; rows land in the caller's array in input order.
    std::vector<sfa_ctx *> shards;
    std::vector<std::unique_ptr<ShardWorker>> workers;  // [shards - 1]: shard r > 0 is driven from workers[r - 1], shard 0 from the caller
    std::vector<int32_t> shard_lo;  // [shards+1] read ranges of the batch submitted with sfa_submit_batch

    int device = 0;
    uint32_t flag = 0;
    int pore = 0;  // sfa_set_pore: 0 R9, 1 R10, 2 RNA004 (the adaptor segmenter of the RNA automatic query start)
    int cu_count = 256;
    // Streams and events of every stage sit here, in front of the buffers: members go in reverse order of declaration, so the
    // buffers are freed while the streams exist, then the events, then stream_long2, stream_long, stream.
    Stream stream;
    Stream stream_long;   // the row strips of long queries run beside the wave kernels of the same batch
    Stream stream_long2;  // ... their groups alternating between two streams (pass 2 of one under pass 1 of the next)
    Event lev[4];  // inputs of the batch ready on `stream` / strips done on `stream_long` / fork and join of `stream_long2`
    Event eev[4];  // sfa_align_raw: event detection start/end, normalisation start/end
    Event ev[6];   // fill start/end, finalize1 end, trace end, end, row strips start
    Event bev[2];  // sfa_align_blow5: record decoding start / end

    // tunables (sfa_set_option)
    int64_t opt_ckpt_interval = 0;           // force the checkpoint interval (power of two >= 4); 0 = auto
    int64_t opt_ckpt_budget = 32ll << 30;    // bytes of HBM the checkpoints of one batch may take
    int64_t opt_ev_parallel = 3;             // sfa_align_raw: bit 0 wave-per-read prefix sums where they are provably exact, bit 1 wave-per-read peak picker where its result is certified
    int64_t opt_zstd_tables = 1;             // device zstd decoder: 1 tables in LDS (at most 4 records per block; measured faster), 0 in the records' scratch areas in HBM
    int64_t opt_min_slice_reads = 65536;    // a batch is only cut into slices of at least this many reads
    int64_t opt_segment_warm = 4;            // query lengths of warm-up in front of a segment
    int64_t opt_column_segments = 0;         // 0 = auto, 1 = off, N = segments per job for small batches (sweep_segment)
    int64_t opt_lane_widening = 0;           // 0 = by batch size; 1, 2, 4 = fixed (rows per lane / w, lanes per read * w)
    int64_t opt_widen_below = 5;             // auto: widen (x4) when the batch has fewer waves per SIMD than this
    int64_t opt_trace_margin = -1;           // steps of head start for pass 2; -1 = qlen_max + 16
    int64_t opt_waves_per_simd = 6;          // target occupancy used when chunking the job list
    int64_t opt_fused_trace = 1;             // 1: pass 2 rides in the fill launch as trailing tickets (fills the drain) where the launch has more tasks than wave slots; 2: always; 0: own launch
    int64_t opt_lds_ckpt = 1;                // 1: rolling checkpoints in LDS where the batch's shapes allow (R <= 16, sDTW); 0: all snapshots to HBM
    int64_t opt_secondary = 0;               // secondary mappings per read, 0..4 (sfa_secondary_rows); > 0 takes the plain two-pass route
    int64_t opt_secondary_strips = 0;        // 1: with opt_secondary > 0, reads beyond SFA_MAX_QUERY events have secondaries too (the row strips keep the lists)
    int64_t opt_prio_unit = 2048;            // longest-remaining-first issue priority of the fill: columns per level, 0 = off
    int64_t opt_spin_limit_ms = 20000;       // bound of every in-launch wait (fused pass 2, pipelined strips); beyond it the batch fails with SFA_EKERNEL
    // test hooks (sfa_set_option refuses them unless SFA_TEST_HOOKS=1 is in the environment)
    int64_t opt_debug_drop_quad = -1;        // the fill tasks of this quad never signal completion
    int64_t opt_debug_drop_strip = -1;       // strip 0 of this long read (job 0) never publishes its progress
    int64_t opt_map_scratch = 2ll << 30;  // bytes of HBM the move matrices of one slice of rows may take
    int64_t opt_map_strips = 0;           // 1: event maps of rows beyond SFA_MAX_QUERY events on the device, in row strips (sdtw_path.hpp)

    ctx::RefModel model;
    ctx::CallerIO io;
    ctx::Status status;
    ctx::WaveKernels wave;
    ctx::FusedLaunch fused;
    ctx::LdsRoute lds;
    ctx::Segments seg;
    ctx::Strips strips;
    ctx::Secondaries sec;
    ctx::RawSignal raw;
    ctx::Blow5 blow5;
    ctx::EventMaps maps;
    ctx::TaskTimes times;
    sfa_profile_t prof{};
    bool prof_pending = false;
    bool in_slice = false;  // align_device is running one slice of a cut-up batch
    std::vector<struct sfa_session *> sessions;  // live sessions of this context (sfa_session.hip); sfa_destroy frees them first (a group
                                                 // context's are its spread sessions: freed before the shards their sub-sessions live on)
};

// ---- internal functions that cross unit boundaries ----
namespace sfa {
void destroy_sessions(sfa_ctx *c);  // sfa_session.hip: every live session of the context (sfa_destroy)
int resolve_profile(sfa_ctx *c);  // sfa_align.hip: timers + error words of the batch submitted last (waits for it)
// core of every align entry point: queries already in HBM, results left in HBM (sfa_align.hip)
int align_device(sfa_ctx *c, const float *d_queries, const int64_t *q_off, int32_t n, struct ResultRow *d_out,
                 struct ResultRow *d_sec = nullptr);  // d_sec: rows of the secondaries (nullptr: the context's d_sec, when the option is on)
// ---- the core of both event-maps entry points (sfa_maps.hip) ----
struct MapRow {  // one row of a call, as the core takes it
    int32_t k = 0;                                             // the caller's number of the row: its map goes to pairs + 2 * map_off[k]
    int32_t query = -1, job = 0, col_st = 0, m = 0, qlen = 0;  // m = 0: nothing to write for this row
};
// The band of row k in columns of its strand's own array: the flip and offset of src/sigfish.c:971-975 undone.  qlen: events of
// the query the row aligns; gap: the pairs map_off leaves for it.  SFA_EINVAL for a row that is not one of this reference (what:
// ends the message, "a row of ..."), SFA_ERANGE for a gap too small
int map_row_band(const sfa_ctx *c, const sfa_result_t &r, int32_t k, int64_t qlen, int64_t gap, const char *who, const char *what, MapRow *b);
// Maps of band[0..n) on the context's device and stream, into the caller's pairs.  The query of a row lies at d_queries +
// q_off[row.query], row.qlen events in DP order (reversed: in event order, the DP takes them back to front); q_off[n_q_off] is
// host memory.  Scratch: sc.  Rows beyond the "map_scratch_bytes" budget take the host routine; so do rows beyond SFA_MAX_QUERY
// events unless "map_strips" is on, which runs them in row strips.
int event_maps_core(sfa_ctx *c, ctx::MapScratch &sc, const float *d_queries, const int64_t *q_off, size_t n_q_off, bool reversed, const MapRow *band, int32_t n,
                    const int64_t *map_off, int32_t *pairs, int32_t *n_on_host);
// contiguous read range of shard r: [r*n/G, (r+1)*n/G)
inline void shard_ranges(int32_t n, size_t g, std::vector<int32_t> *lo) {
    lo->resize(g + 1);
    for (size_t r = 0; r <= g; ++r) (*lo)[r] = static_cast<int32_t>(static_cast<int64_t>(n) * static_cast<int64_t>(r) / static_cast<int64_t>(g));
}
// run fn(shard index) for every shard, each on the shard's own host thread (HIP's current device and sfa_last_error are
// per thread), shard 0 on the caller's; the first failure's code and message become the caller's
template <typename F>
int for_each_shard(sfa_ctx *g, F fn) {
    const size_t G = g->shards.size();
    for (size_t r = 1; r < G; ++r) g->workers[r - 1]->post([&fn, r] { return fn(r); });
    int rc = fn(0);
    std::string msg = rc ? last_error_slot() : std::string();
    for (size_t r = 1; r < G; ++r) {  // (always all of them: fn and what it captures must outlive every worker's job)
        const auto res = g->workers[r - 1]->wait();
        if (res.first && !rc) {
            rc = res.first;
            msg = res.second;
        }
    }
    if (rc) last_error_slot() = msg;
    return rc;
}
// a call over n reads split the way every entry point splits it: fn(r, lo, hi) for every shard r whose range [lo, hi) is not
// empty (for_each_shard); *ranges (if given) keeps the split
template <typename F>
int for_each_shard_range(sfa_ctx *g, int32_t n, F fn, std::vector<int32_t> *ranges = nullptr) {
    std::vector<int32_t> own;
    std::vector<int32_t> &lo = ranges ? *ranges : own;
    shard_ranges(n, g->shards.size(), &lo);
    return for_each_shard(g, [&](size_t r) { return lo[r] == lo[r + 1] ? static_cast<int>(SFA_OK) : fn(r, lo[r], lo[r + 1]); });
}
}  // namespace sfa
