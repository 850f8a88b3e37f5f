// sfa_align.hip -- the alignment stage behind the C-ABI (include/sigfish_amd.h): replaces the reference's accelerator hook
// align_db() (src/sigfish.c:1003-1015).  Host work: group reads into "quads" (reads of one length class share a wavefront;
// sfa_plan.hpp), pick the rows-per-lane class, size the checkpoint interval, launch fill (+ pass 2 by ticket, or fill ->
// finalize -> trace -> finalize), row strips for queries beyond 2048 events, and hand back one row per read in input order.
// Both paths have one shape: a plan that is plain C++ (sfa_plan.hpp: plan_batch + choose_route, plan_long_reads), then stages that
// hand it on -- stage_and_reserve / batch_args / enqueue_pass1, 2 for the wave kernels, stage_long / long_args / enqueue_long_group
// for the row strips -- under enqueue_batch.
#define SFA_DEFINE_FINALIZE_KERNEL  // (of sdtw_kernels.hpp and sdtw_strips.hpp: this unit holds the plain kernels)
#include "sfa_ctx.hpp"
#include "sdtw_instances.hpp"
#include "sdtw_strips.hpp"

using sfa::DpArgs;
using sfa::FinalizeArgs;
using sfa::Route;
using sfa::SecArgs;
using sfa::ResultRow;
using sfa::align_device;
using sfa::for_each_shard;
using sfa::for_each_shard_range;
using sfa::resolve_profile;

namespace {

// f(std::integral_constant<int, R>()) for the rows-per-lane class R (4, 8, 16, 32; at most Cap) of a batch whose widest
// class has maxr rows per lane
template <int Cap, typename F>
void by_rows(int maxr, F f) {
    if constexpr (Cap >= 32) {
        if (maxr >= 32) return f(std::integral_constant<int, 32>());
    }
    if (maxr >= 16) return f(std::integral_constant<int, 16>());
    if (maxr >= 8) return f(std::integral_constant<int, 8>());
    f(std::integral_constant<int, 4>());
}

// f(std::true_type()) for --dtw-std (the kernels' STD argument), else f(std::false_type())
template <typename F>
void by_std(bool std_dtw, F f) {
    if (std_dtw)
        f(std::true_type());
    else
        f(std::false_type());
}

// ---- reads of more than SFA_MAX_QUERY events, row strips (sdtw_strips.hpp): plan -> staging and scratch -> argument blocks -> launches
// Pass 1, one wave per (read, job, strip), sweeps the query in strips of 64 x R rows, cost only, handing the last row of a strip to
// the next one through HBM; the strip finalize names each read's winning (job, cell, score); pass 2, one wave per read, traces the
// winning job strip by strip from the last one upwards with start-column tracking.  Every count, offset and size, the checkpoint
// interval, the groups and the limit of the waits are sfa::plan_long_reads' (sfa_plan.hpp: no HIP in it, tests/c/long_plan.cpp).

// "secondary_strips": the long reads of a batch keep their candidate lists (it has an effect only while "secondary" is 1..4)
bool strip_secondaries(const sfa_ctx *c) { return c->opt_secondary > 0 && c->opt_secondary_strips != 0; }

// staging and every scratch buffer of the long reads, the plan into the page-locked staging area and up, on `st`
int stage_long(sfa_ctx *c, const sfa::LongPlan &lp, hipStream_t st) {
    const int sets = lp.two_sets ? 2 : 1;
    const size_t n_long = static_cast<size_t>(lp.n_long());
    int rc;
    if ((rc = c->strips.reserve_staging(lp.sg.bytes))) return rc;
    if ((rc = c->strips.reserve(lp.prog_bytes * sets, lp.bndc_floats * sets, lp.lck_floats * sets, lp.n_part, n_long, st))) return rc;
    if (strip_secondaries(c)) {  // (no rank has been traced yet: -1)
        if ((rc = c->strips.reserve_secondary(lp.sec_list_words, lp.sec_rank_words))) return rc;
        HIP_TRY(hipMemsetAsync(c->strips.d_lranks.as<int32_t>() + lp.sec_traced(), 0xff, 4 * lp.sec_traced_words(), st));
    }
#ifdef SFA_TASK_TIMES
    if ((rc = c->times.d_ltimes.reserve(24 * lp.n_part * lp.max_strips))) return rc;  // (room for any group: no growth under one that is running)
#endif
    char *hs = c->strips.h_long.as<char>();
    memcpy(hs + lp.sg.reads, lp.reads.data(), sizeof(int32_t) * n_long);
    memcpy(hs + lp.sg.bnd, lp.bnd_off.data(), sizeof(int64_t) * lp.bnd_off.size());
    memcpy(hs + lp.sg.ck, lp.ck_off.data(), sizeof(int64_t) * lp.ck_off.size());
    memcpy(hs + lp.sg.soff, lp.strip_off.data(), sizeof(int32_t) * lp.strip_off.size());
    HIP_TRY(hipMemcpyAsync(c->strips.d_long.p, hs, lp.sg.bytes, hipMemcpyHostToDevice, st));
    return SFA_OK;
}

struct LongWinners {  // d_lwin, [5][n_long] words: a group's part of every row, from its first read g0
    int32_t *w_job, *w_ws;
    float *w_score;
    int32_t *t_st, *t_end;
    LongWinners(int32_t *win, size_t n_long, size_t g0)
        : w_job(win + g0), w_ws(win + n_long + g0), w_score(reinterpret_cast<float *>(win + 2 * n_long + g0)), t_st(win + 3 * n_long + g0), t_end(win + 4 * n_long + g0) {}
};

struct LongRanks {  // d_lranks (LongPlan::sec_rank): rank k of a group's reads, from its first read g0
    int32_t *job, *col;
    float *score;
    int32_t *st, *end;
    LongRanks(int32_t *w, const sfa::LongPlan &lp, int k, int32_t g0)
        : job(w + lp.sec_rank(lp.kSecJob, k, g0)), col(w + lp.sec_rank(lp.kSecCol, k, g0)), score(reinterpret_cast<float *>(w + lp.sec_rank(lp.kSecScore, k, g0))),
          st(w + lp.sec_rank(lp.kSecStart, k, g0)), end(w + lp.sec_rank(lp.kSecEnd, k, g0)) {}
};

struct LongArgs {  // the argument blocks of a group: pass 1 and pass 2, the strip finalize; with secondaries their lists and merge
    sfa::StripArgs sa{};
    sfa::StripFinalizeArgs fa{};
    int32_t *p_top5 = nullptr;  // nullptr: no secondaries for the long reads
    sfa::StripSecArgs xa{};
};

// the secondaries' finalize over long reads g0 ... g0 + gn - 1 of the batch (sa: any group's block, for what all groups share)
sfa::StripSecArgs strip_sec_args(const sfa_ctx *c, const sfa::LongPlan &lp, int32_t g0, int32_t gn, ResultRow *d_sec) {
    const LongRanks r(c->strips.d_lranks.as<int32_t>(), lp, 0, g0);
    sfa::StripSecArgs xa{};
    xa.reads = reinterpret_cast<const int32_t *>(c->strips.d_long.as<char>() + lp.sg.reads) + g0;
    xa.p_top5 = c->strips.d_lp5.as<int32_t>() + static_cast<size_t>(g0) * c->model.n_jobs * sfa::kSecListWords;
    xa.bad = c->status.d_bad.as<uint8_t>();
    xa.s_job = r.job;
    xa.s_ws = r.col;
    xa.s_score = r.score;
    xa.t_st = r.st;
    xa.t_end = r.end;
    xa.ref = c->model.tables();
    xa.sec = d_sec;
    xa.n_long = gn;
    xa.n_total = lp.n_long();
    xa.n_jobs = c->model.n_jobs;
    xa.n_sec = static_cast<int32_t>(c->opt_secondary);
    return xa;
}

// the finalize of the group that sa describes: what the two blocks share comes from sa
sfa::StripFinalizeArgs strip_finalize_args(const sfa_ctx *c, const sfa::StripArgs &sa, const LongWinners &w, ResultRow *d_out) {
    sfa::StripFinalizeArgs fa{};
    fa.reads = sa.reads;
    fa.p_best = sa.p_best;
    fa.p_second = sa.p_second;
    fa.p_end = sa.p_end;
    fa.ref = c->model.tables();
    fa.w_job = w.w_job;
    fa.w_ws = w.w_ws;
    fa.w_score = w.w_score;
    fa.t_st = sa.t_st;
    fa.t_end = sa.t_end;
    fa.out = d_out;
    fa.bad = c->status.d_bad.as<uint8_t>();
    fa.n_long = sa.n_long;
    fa.n_jobs = sa.n_jobs;
    return fa;
}

LongArgs long_args(sfa_ctx *c, const sfa::LongPlan &lp, int32_t gi, const float *d_queries, const int64_t *d_q_off, ResultRow *d_out, ResultRow *d_sec) {
    const int32_t g0 = lp.begin(gi), gn = lp.size(gi), n_jobs = c->model.n_jobs;
    const int set = lp.set(gi);
    const char *ds = c->strips.d_long.as<char>();
    const LongWinners w(c->strips.d_lwin.as<int32_t>(), static_cast<size_t>(lp.n_long()), static_cast<size_t>(g0));
    LongArgs a;
    sfa::StripArgs &sa = a.sa;
    sa.queries = d_queries;
    sa.q_off = d_q_off;
    sa.reads = reinterpret_cast<const int32_t *>(ds + lp.sg.reads) + g0;
    sa.ref = c->model.d_ref.as<float>();
    sa.job_off = c->model.d_job_off.as<int64_t>();
    sa.job_len = c->model.d_job_len.as<int32_t>();
    sa.bnd_off = reinterpret_cast<const int64_t *>(ds + lp.sg.bnd);
    sa.bnd_cost = c->strips.d_bndc.as<float>() + set * lp.bndc_floats;
    sa.bnd_stride = lp.bnd_stride;
    sa.p_best = c->strips.d_lbest.as<float>() + static_cast<size_t>(g0) * n_jobs;
    sa.p_second = c->strips.d_lsecond.as<float>() + static_cast<size_t>(g0) * n_jobs;
    sa.p_end = c->strips.d_lend.as<int32_t>() + static_cast<size_t>(g0) * n_jobs;
    sa.w_job = w.w_job;
    sa.w_ws = w.w_ws;
    sa.w_score = w.w_score;
    sa.t_st = w.t_st;
    sa.t_end = w.t_end;
    sa.ck = c->strips.d_lck.as<float>() + set * lp.lck_floats;
    sa.ck_off = reinterpret_cast<const int64_t *>(ds + lp.sg.ck);
    sa.ck_shift = lp.ck_shift;
    sa.max_strips = lp.max_strips;
    sa.trace_margin = static_cast<int32_t>(c->opt_trace_margin);
    sa.n_long = gn;
    sa.n_jobs = n_jobs;
    sa.rev_query = ((c->flag & SFA_RNA) && !(c->flag & SFA_INV)) ? 1 : 0;
    sa.strip_off = reinterpret_cast<const int32_t *>(ds + lp.sg.soff) + lp.off_word(gi);
    sa.progress = reinterpret_cast<int32_t *>(c->strips.d_lprog.as<char>() + set * lp.prog_bytes);
    sa.ticket = c->strips.d_lticket.as<unsigned>() + set * 16;  // (words 8.. of a set's 64 bytes: where a dropped strip publishes, see strip_pipe_task)
    sa.err = c->status.dev()->err;
    sa.spin_limit = lp.limit_ms * 100000;  // 100 MHz ticks
    c->strips.strip_limit_ms = lp.limit_ms;
    sa.debug_drop_strip = (c->opt_debug_drop_strip >= g0 && c->opt_debug_drop_strip < g0 + gn) ? static_cast<int32_t>(c->opt_debug_drop_strip - g0) : -1;
#ifdef SFA_TASK_TIMES
    sa.task_times = c->times.d_ltimes.as<unsigned long long>();
    c->times.n_ltimes = static_cast<int64_t>(lp.strips_of(gi)) * n_jobs;
#endif
    a.fa = strip_finalize_args(c, sa, w, d_out);
    if (strip_secondaries(c) && d_sec) {
        a.p_top5 = c->strips.d_lp5.as<int32_t>() + static_cast<size_t>(g0) * n_jobs * sfa::kSecListWords;
        a.xa = strip_sec_args(c, lp, g0, gn, d_sec);
    }
    return a;
}

// a group of `strips` strips on its stream: pass 1 (one wave per (job, read, strip), tickets in that order), winners, pass 2, rows.
// With secondaries pass 1 is the kernel that keeps the lists, and behind the rows come the merge of the lists and pass 2 once more
// per rank 1..n_sec, the same kernel pointed at that rank's (job, column, score) and columns: the boundary rows and checkpoints of the
// group stay where they are until the next group of this stream starts.  (The secondaries' rows: enqueue_batch, behind the join.)
int enqueue_long_group(const LongArgs &a, int64_t strips, bool std_dtw, hipStream_t st) {
    const sfa::StripArgs &sa = a.sa;
    sfa::StripFinalizeArgs fa = a.fa;
    const int64_t waves = strips * sa.n_jobs;
    const dim3 block(256), gridp(static_cast<unsigned>((waves + 3) / 4)), grid2((sa.n_long + 3) / 4), fgrid((sa.n_long + 63) / 64), fblock(64);
    HIP_TRY(hipMemsetAsync(sa.progress, 0, sizeof(int32_t) * static_cast<size_t>(sa.n_long) * sa.n_jobs * sa.max_strips, st));
    HIP_TRY(hipMemsetAsync(sa.ticket, 0, 4, st));
    if (a.p_top5)
        by_std(std_dtw, [&](auto S) { hipLaunchKernelGGL((sfa::sdtw_strip_sec_pipe_kernel<S>), gridp, block, 0, st, sa, a.p_top5); });
    else
        by_std(std_dtw, [&](auto S) { hipLaunchKernelGGL((sfa::sdtw_strip_pipe_kernel<S>), gridp, block, 0, st, sa); });
    KERNEL_TRY();
    fa.mode = 1;
    hipLaunchKernelGGL(sfa::sdtw_strip_finalize_kernel, fgrid, fblock, 0, st, fa);
    KERNEL_TRY();
    by_std(std_dtw, [&](auto S) { hipLaunchKernelGGL((sfa::sdtw_strip_chain_kernel<S>), grid2, block, 0, st, sa); });
    KERNEL_TRY();
    fa.mode = 2;
    hipLaunchKernelGGL(sfa::sdtw_strip_finalize_kernel, fgrid, fblock, 0, st, fa);
    KERNEL_TRY();
    if (!a.p_top5) return SFA_OK;
    sfa::StripSecArgs xa = a.xa;
    xa.mode = 1;
    hipLaunchKernelGGL(sfa::sdtw_strip_sec_finalize_kernel, fgrid, fblock, 0, st, xa);
    KERNEL_TRY();
    for (int k = 1; k <= xa.n_sec; ++k) {
        const size_t o = static_cast<size_t>(k) * xa.n_total;
        sfa::StripArgs ra = sa;
        ra.w_job = xa.s_job + o;
        ra.w_ws = xa.s_ws + o;
        ra.w_score = xa.s_score + o;
        ra.t_st = xa.t_st + o;
        ra.t_end = xa.t_end + o;
        by_std(std_dtw, [&](auto S) { hipLaunchKernelGGL((sfa::sdtw_strip_chain_kernel<S>), grid2, block, 0, st, ra); });
        KERNEL_TRY();
    }
    return SFA_OK;
}

// The long reads of a batch on `first`, the context's second stream, beside the wave kernels of the batch; it writes the rows of
// these reads, which the wave kernels' finalize leaves alone.  Reads are taken in groups whose boundary rows and checkpoints fit
// the checkpoint budget -- and, when there are enough of them, in two groups on two streams with two sets of scratch: pass 2 of a
// group is one wave per read (0.8 waves per SIMD for 3 125 reads: bound by one wave's dependent chain, 12 ms at 8 000 events) and
// runs beside the other group's work instead of behind everything.  Measured on one box, ms per step at 3 000 / 8 000 events: one
// group 99.9 / 103.5, two 97.4 / 99.2, four 104.7 / 118.8 (more drains than they hide): profiles/r04_logs/strips_groups_ab*.log,
// rejected_strip_pass2_rows_in_lds_three_waves.log.
int align_long(sfa_ctx *c, const sfa::LongPlan &lp, const float *d_queries, const int64_t *d_q_off, ResultRow *d_out, ResultRow *d_sec, hipStream_t first) {
    if (int rc = stage_long(c, lp, first)) return rc;
    if (lp.two_sets) {  // the second stream starts behind the staging upload (and whatever `first` waited for)
        HIP_TRY(hipEventRecord(c->lev[2], first));
        HIP_TRY(hipStreamWaitEvent(c->stream_long2, c->lev[2], 0));
    }
    for (int32_t gi = 0; gi < lp.n_groups; ++gi) {
        const LongArgs a = long_args(c, lp, gi, d_queries, d_q_off, d_out, d_sec);
        if (int rc = enqueue_long_group(a, lp.strips_of(gi), (c->flag & SFA_DTW) != 0, lp.set(gi) ? c->stream_long2 : first)) return rc;
    }
    if (lp.two_sets) {  // whoever waits for `first` waits for both
        HIP_TRY(hipEventRecord(c->lev[3], c->stream_long2));
        HIP_TRY(hipStreamWaitEvent(first, c->lev[3], 0));
    }
    return SFA_OK;
}

// A batch so large that its checkpoints only fit the budget at a long interval (a long pass 2) is cut into slices
// of contiguous reads that keep the interval short; slices of >= 64 Ki reads still fill the chip.  Slices run one
// after the other (each is planned and staged on its own), so such a call is synchronous.

int align_sliced(sfa_ctx *c, const float *d_queries, const int64_t *q_off, int32_t n, ResultRow *d_out, ResultRow *d_sec, int32_t slices) {
    sfa_profile_t sum{};
    for (int32_t s = 0; s < slices; ++s) {
        const int32_t lo = static_cast<int32_t>(static_cast<int64_t>(n) * s / slices);
        const int32_t hi = static_cast<int32_t>(static_cast<int64_t>(n) * (s + 1) / slices);
        c->in_slice = true;
        int rc = align_device(c, d_queries, q_off + lo, hi - lo, d_out + lo, d_sec ? d_sec + 4 * static_cast<int64_t>(lo) : nullptr);  // q_off holds absolute offsets into d_queries
        c->in_slice = false;
        if (rc) return rc;
        if ((rc = resolve_profile(c))) return rc;  // waits for the slice: the staging area is reused by the next one
        sum.fill_ms += c->prof.fill_ms;
        sum.trace_ms += c->prof.trace_ms;
        sum.finalize_ms += c->prof.finalize_ms;
        sum.total_ms += c->prof.total_ms;
        sum.cells += c->prof.cells;
        sum.fill_launches += c->prof.fill_launches;
        sum.ckpt_interval = std::max(sum.ckpt_interval, c->prof.ckpt_interval);
        sum.ckpt_bytes = std::max(sum.ckpt_bytes, c->prof.ckpt_bytes);
        sum.trace_margin = std::max(sum.trace_margin, c->prof.trace_margin);
        sum.lds_ckpt = std::max(sum.lds_ckpt, c->prof.lds_ckpt);
        sum.fused_trace = std::max(sum.fused_trace, c->prof.fused_trace);
        sum.n_tasks += c->prof.n_tasks;
        sum.n_chunks = std::max(sum.n_chunks, c->prof.n_chunks);
        sum.non_finite_reads += c->prof.non_finite_reads;
        sum.lck_fallbacks += c->prof.lck_fallbacks;
        sum.lck_from_scratch += c->prof.lck_from_scratch;
    }
    c->prof = sum;
    return SFA_OK;
}

// ---- one batch of the wave kernels: plan -> route -> staging and scratch -> argument blocks -> launches -------------------

bool fused(Route r) { return r == Route::LdsFused || r == Route::Fused32; }  // pass 2 rides in the fill launch
bool lds(Route r) { return r == Route::Lds || r == Route::LdsFused; }        // the fill keeps its checkpoints in LDS

sfa::PlanParams plan_params(const sfa_ctx *c) {
    sfa::PlanParams pp;
    pp.n_sims = static_cast<int64_t>(c->cu_count) * 4;
    pp.waves_per_simd = c->opt_waves_per_simd;
    pp.ckpt_interval = c->opt_ckpt_interval;
    pp.ckpt_budget_bytes = c->opt_ckpt_budget;
    pp.trace_margin = c->opt_trace_margin;
    pp.lane_widening = c->opt_lane_widening;
    pp.widen_below = c->opt_widen_below;
    pp.column_segments = c->opt_column_segments;
    pp.segment_warm_windows = c->opt_segment_warm;
    pp.std_dtw = (c->flag & SFA_DTW) != 0;
    pp.span_sixteenths = c->wave.span_sixteenths;
    // what follows from the route: secondaries take the plain two-pass route (no LDS checkpoints, no column segments); std_dtw
    // has no column segments (its first row is cumulative: no finite memory), nor has the re-run of a batch whose hand-overs failed
    pp.allow_segments = !pp.std_dtw && !c->seg.no_segments_once && c->opt_secondary == 0;
    pp.lds_ckpt = c->opt_secondary > 0 ? 0 : static_cast<int>(c->opt_lds_ckpt);
    return pp;
}

// staging layout: q_off[n+1] (at 0) | order[4*n_quads] | quad_qlen[n_quads] | slot[n] | chunk_begin[n_chunks+1] | job_ck_off[n_jobs+1]
struct Staging {
    size_t order, qq, slot, chunk, ckoff, bytes;
    Staging(int32_t n, const sfa::BatchPlan &p, int32_t n_jobs) {
        order = sizeof(int64_t) * (n + 1);
        qq = order + sizeof(int32_t) * 4 * std::max(p.n_quads, 1);
        slot = qq + sizeof(int32_t) * std::max(p.n_quads, 1);
        chunk = slot + sizeof(int32_t) * n;
        ckoff = chunk + sizeof(int32_t) * (p.n_chunks + 1);
        bytes = ckoff + sizeof(int32_t) * (n_jobs + 1);
    }
};

// every scratch buffer of the batch (each on the conditions of its route), and the plan into the page-locked staging area
int stage_and_reserve(sfa_ctx *c, const int64_t *q_off, int32_t n, Route route, const Staging &sg) {
    const sfa::BatchPlan &plan = c->wave.plan;
    const int32_t n_quads = plan.n_quads, n_chunks = plan.n_chunks, n_jobs = c->model.n_jobs;
    const size_t n_part = static_cast<size_t>(std::max(n_quads, 1)) * n_chunks * 4, nr = static_cast<size_t>(n);
    int rc;
    if ((rc = c->wave.reserve(sg.bytes, n_part, nr, plan.ck_floats)) || (rc = c->status.reserve(nr))) return rc;
    if (c->opt_secondary > 0 && (rc = c->sec.reserve(n_part, nr))) return rc;
    if (fused(route) && (rc = c->fused.reserve(static_cast<size_t>(std::max(n_quads, 1))))) return rc;
    if (lds(route) && (rc = c->lds.reserve(n_part, nr))) return rc;
    if (route == Route::Segments && (rc = c->seg.reserve(plan, n_jobs))) return rc;
    char *hs = c->wave.h_stage.as<char>();
    memcpy(hs, q_off, sizeof(int64_t) * (n + 1));
    memcpy(hs + sg.order, plan.order.data(), sizeof(int32_t) * plan.order.size());
    memcpy(hs + sg.qq, plan.quad_qlen.data(), sizeof(int32_t) * plan.quad_qlen.size());
    memcpy(hs + sg.slot, plan.slot_of_read.data(), sizeof(int32_t) * n);
    memcpy(hs + sg.chunk, plan.chunk_begin.data(), sizeof(int32_t) * (n_chunks + 1));
    memcpy(hs + sg.ckoff, plan.job_ck_off.data(), sizeof(int32_t) * (n_jobs + 1));
#ifdef SFA_TASK_TIMES
    if ((rc = c->times.d_times.reserve(24 * static_cast<size_t>(std::max(n_quads * n_chunks, 1))))) return rc;
    c->times.n_times = n_quads * n_chunks;
#endif
    return SFA_OK;
}

// The kernels' argument blocks: pass 1 (and, one task per quad, pass 2), the finalize, the secondaries' merge
struct BatchArgs {
    DpArgs da{};
    FinalizeArgs fz{};
    SecArgs sa{};
};

BatchArgs batch_args(sfa_ctx *c, const float *d_queries, int32_t n, ResultRow *d_out, ResultRow *d_sec, Route route, const Staging &sg,
                     bool has_long) {
    const sfa::BatchPlan &plan = c->wave.plan;
    const int32_t n_quads = plan.n_quads, n_chunks = plan.n_chunks, n_jobs = c->model.n_jobs;
    const char *ds = c->wave.d_stage.as<char>();
    BatchArgs a;
    DpArgs &da = a.da;
    da.queries = d_queries;
    da.q_off = reinterpret_cast<const int64_t *>(ds);
    da.order = reinterpret_cast<const int32_t *>(ds + sg.order);
    da.quad_qlen = reinterpret_cast<const int32_t *>(ds + sg.qq);
    da.ref = c->model.d_ref.as<float>();
    da.job_off = c->model.d_job_off.as<int64_t>();
    da.job_len = c->model.d_job_len.as<int32_t>();
    da.chunk_begin = reinterpret_cast<const int32_t *>(ds + sg.chunk);
    da.job_ck_off = reinterpret_cast<const int32_t *>(ds + sg.ckoff);
    da.ck = c->wave.d_ck.as<float>();
    da.p_best = c->wave.d_pbest.as<float>();
    da.p_end = c->wave.d_pend.as<int32_t>();
    da.p_job = c->wave.d_pjob.as<int32_t>();
    da.p_second = c->wave.d_psecond.as<float>();
    da.w_job = c->wave.d_wjob.as<int32_t>();
    da.w_end = c->wave.d_wend.as<int32_t>();
    da.w_score = c->wave.d_wscore.as<float>();
    da.n_reads_total = n;
    da.n_cls = static_cast<int32_t>(plan.classes.size());
    for (int i = 0; i < da.n_cls; ++i) {
        da.cls[i].R = plan.classes[i].R;
        da.cls[i].lanes = plan.classes[i].lanes;
        da.cls[i].quad_base = plan.classes[i].quad_base;
        da.cls[i].n_quads = plan.classes[i].n_quads;
        da.cls[i].task_base = plan.classes[i].quad_base * n_chunks;  // classes are contiguous in quad order
        da.cls[i].ck_base = plan.classes[i].ck_base;
    }
    da.n_chunks = n_chunks;
    da.n_tasks = n_quads * n_chunks;
    da.rev_query = ((c->flag & SFA_RNA) && !(c->flag & SFA_INV)) ? 1 : 0;
    da.ck_shift = plan.ck_shift;
    da.trace_margin = plan.trace_margin;
    da.n_seg = plan.n_seg;
    da.warm_windows = plan.warm_windows;
    da.n_jobs = n_jobs;
    da.verify_planes = plan.max_R + 1;
    da.verify = c->seg.d_verify.as<float>();
    da.seg_fail = c->seg.d_segfail.as<int32_t>();
    da.best_rec = c->lds.d_bestrec.as<float>();
    da.best_e = c->lds.d_beste.as<int32_t>();
    da.g_best = c->lds.d_gbest.as<unsigned>();
    da.w_chunk = c->wave.d_wchunk.as<int32_t>();
    da.best_planes = sfa::kLdsCkPlanes;
    da.ticket = c->fused.d_ticket.as<unsigned>();
    da.quad_done = c->fused.d_quaddone.as<int32_t>();
    da.n_quads_total = n_quads;
    const sfa::RefTables ref = c->model.tables();
    da.job_contig = ref.job_contig;  // (DpArgs keeps its own words: the DP kernels were built around them)
    da.job_strand = ref.job_strand;
    da.ref_len = ref.ref_len;
    da.ref_st_offset = ref.ref_st_offset;
    da.bad = c->status.d_bad.as<uint8_t>();
    da.out = d_out;
    da.span_hist = route == Route::Fused32 ? c->status.dev()->span_hist : nullptr;  // (the LDS route caps its head start instead)
    da.prio_unit = static_cast<int32_t>(c->opt_prio_unit);
    da.started = c->wave.d_started.as<unsigned>();
    da.err = c->status.dev()->err;
    da.lck_stats = &c->status.dev()->lck_fallbacks;  // (and lck_from_scratch behind it)
    {   // a pass-2 wave legitimately waits for as long as one fill task of its quad runs: never less than ~5x that (1 us per
        // column of the longest chunk, against 0.2 measured), however small the option -- a 250 Mb strand is minutes, not a hang
        int64_t longest = 0;
        for (int32_t ch = 0; ch < n_chunks; ++ch) {
            int64_t cols = 0;
            for (int32_t j = plan.chunk_begin[ch]; j < plan.chunk_begin[ch + 1] && j < n_jobs; ++j) cols += c->model.h_job_len[j];
            longest = std::max(longest, cols);
        }
        da.spin_limit = std::max<int64_t>(c->opt_spin_limit_ms, longest / 1000) * 100000;  // 100 MHz ticks
        c->wave.quad_limit_ms = da.spin_limit / 100000;
    }
    da.debug_drop_quad = static_cast<int32_t>(c->opt_debug_drop_quad);
    da.p_top5 = route == Route::Secondary ? c->sec.d_p5.as<int32_t>() : nullptr;
    da.self = fused(route) ? c->fused.d_args.as<DpArgs>() : nullptr;
#ifdef SFA_TASK_TIMES
    da.task_times = c->times.d_times.as<unsigned long long>();
#endif

    FinalizeArgs &fz = a.fz;
    fz.slot_of_read = reinterpret_cast<const int32_t *>(ds + sg.slot);
    fz.p_best = da.p_best;
    fz.p_end = da.p_end;
    fz.p_job = da.p_job;
    fz.p_second = da.p_second;
    fz.ref = ref;
    fz.w_job = da.w_job;
    fz.w_end = da.w_end;
    fz.w_score = da.w_score;
    fz.w_chunk = da.w_chunk;
    fz.t_st = c->wave.d_tst.as<int32_t>();
    fz.out = d_out;
    fz.bad = da.bad;
    fz.q_off = da.q_off;
    fz.max_query = has_long ? sfa::kMaxQuery : 0;
    fz.n_reads = n;
    fz.n_chunks = n_chunks;
    fz.span_hist = c->status.dev()->span_hist;

    if (c->opt_secondary > 0) {
        SecArgs &sa = a.sa;
        sa.slot_of_read = fz.slot_of_read;
        sa.p_top5 = c->sec.d_p5.as<int32_t>();
        sa.bad = fz.bad;
        sa.q_off = fz.q_off;
        sa.max_query = fz.max_query;
        sa.n_reads = n;
        sa.n_chunks = n_chunks;
        sa.s_job = c->sec.d_swin.as<int32_t>();
        sa.s_end = sa.s_job + 5 * static_cast<size_t>(n);
        sa.s_score = reinterpret_cast<float *>(sa.s_end + 5 * static_cast<size_t>(n));
        sa.t_st = c->sec.d_sts.as<int32_t>();
        sa.ref = ref;
        sa.sec = d_sec;
        sa.n_sec = static_cast<int32_t>(c->opt_secondary);
    }
    return a;
}

int launch_finalize(FinalizeArgs fz, int mode, hipStream_t st) {
    fz.mode = mode;
    hipLaunchKernelGGL(sfa::sdtw_finalize_kernel, dim3((fz.n_reads + 255) / 256), dim3(256), 0, st, fz);
    KERNEL_TRY();
    return SFA_OK;
}

// Pass 1 of the route, with what it needs in front of it and behind it.  The LDS routes cap the rows at 16; the segment fill has
// no STD variant (std_dtw has no column segments); the fused grid is the fill tasks followed by one pass-2 ticket per quad.
int enqueue_pass1(sfa_ctx *c, Route route, const BatchArgs &a, hipStream_t st) {
    if (route == Route::NoQuads) return SFA_OK;
    const DpArgs &da = a.da;
    const int32_t n_quads = da.n_quads_total;
    if (lds(route))
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->lds.d_gbest.p), 0x7f800000, static_cast<size_t>(da.n_reads_total), st));  // +inf: no score seen yet
    if (fused(route)) {
        HIP_TRY(hipMemsetAsync(c->fused.d_ticket.p, 0, 4, st));
        HIP_TRY(hipMemsetAsync(c->fused.d_quaddone.p, 0, 4 * static_cast<size_t>(n_quads), st));
        if (int rc = launch_finalize(a.fz, 3, st)) return rc;  // rows of the reads in no quad; every other row is written by the launch's pass-2 waves
        HIP_TRY(hipMemcpyAsync(c->fused.d_args.p, &da, sizeof(DpArgs), hipMemcpyHostToDevice, st));  // (pageable source: staged before the call returns)
    }
    const int maxr = c->wave.plan.max_R;
    const dim3 block(256), grid((da.n_tasks + 3) / 4), fgrid(static_cast<unsigned>((da.n_tasks + 3) / 4 + (n_quads + 3) / 4));
    by_std((c->flag & SFA_DTW) != 0, [&](auto S) {
        if (route == Route::Segments)
            by_rows<32>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_fill_kernel<R, false, true>), grid, block, 0, st, da); });
        else if (route == Route::Lds)
            by_rows<16>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_fill_kernel<R, S, false, true>), grid, block, 0, st, da); });
        else if (route == Route::LdsFused)
            by_rows<16>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_fill_kernel<R, S, false, true, true>), fgrid, block, 0, st, da); });
        else if (route == Route::Fused32)
            hipLaunchKernelGGL((sfa::sdtw_fill_kernel<32, false, false, false, true>), fgrid, block, 0, st, da);
        else if (route == Route::Secondary)
            by_rows<32>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_sec_fill_kernel<R, S>), grid, block, 0, st, da); });
        else  // Route::TwoPass
            by_rows<32>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_fill_kernel<R, S>), grid, block, 0, st, da); });
    });
    KERNEL_TRY();
    if (route == Route::Segments) {  // every hand-over between consecutive segments: assumed state == reached state?
        HIP_TRY(hipMemsetAsync(c->seg.d_segfail.p, 0, 4 * static_cast<size_t>(n_quads), st));
        const int64_t waves = static_cast<int64_t>(n_quads) * da.n_jobs * (da.n_seg - 1);
        hipLaunchKernelGGL(sfa::sdtw_verify_kernel, dim3(static_cast<unsigned>((waves + 3) / 4)), dim3(256), 0, st, da, n_quads);
        KERNEL_TRY();
    }
    return SFA_OK;
}

// the pass-2 kernel of the route for the winners named by ta (w_job, w_end, w_score): start columns to out_st
void launch_pass2(sfa_ctx *c, Route route, DpArgs ta, int32_t *out_st, hipStream_t st) {
    for (int i = 0; i < ta.n_cls; ++i) ta.cls[i].task_base = ta.cls[i].quad_base;  // one task per quad
    ta.n_tasks = ta.n_quads_total;
    const int maxr = c->wave.plan.max_R;
    const dim3 grid((ta.n_tasks + 3) / 4), block(256);
    by_std((c->flag & SFA_DTW) != 0, [&](auto S) {
        if (lds(route))
            by_rows<16>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_trace_kernel<R, S, true>), grid, block, 0, st, ta, out_st); });
        else
            by_rows<32>(maxr, [&](auto R) { hipLaunchKernelGGL((sfa::sdtw_trace_kernel<R, S>), grid, block, 0, st, ta, out_st); });
    });
}

// From the end of the fill (ev[1]) to complete rows: finalize -> (ev[2]) pass 2 -> (ev[3]) finalize; after a fused fill launch
// the rows are complete already
int enqueue_pass2(sfa_ctx *c, Route route, const BatchArgs &a, hipStream_t st) {
    const bool own_launch = route != Route::NoQuads && !fused(route);
    if (int rc = fused(route) ? SFA_OK : launch_finalize(a.fz, 1, st)) return rc;
    HIP_TRY(hipEventRecord(c->ev[2], st));
    if (own_launch) {
        launch_pass2(c, route, a.da, c->wave.d_tst.as<int32_t>(), st);
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(c->ev[3], st));
    return own_launch ? launch_finalize(a.fz, 2, st) : SFA_OK;
}

// merge the chunks' lists, trace candidates 1..n_sec, write their rows (the long reads' rows: valid = 0; with "secondary_strips"
// enqueue_batch writes them again behind the join with the row strips)
int enqueue_secondaries(sfa_ctx *c, Route route, const BatchArgs &a, hipStream_t st) {
    SecArgs sa = a.sa;
    const int32_t n = sa.n_reads;
    const dim3 fgrid((n + 255) / 256), fblock(256);
    sa.mode = 1;
    hipLaunchKernelGGL(sfa::sdtw_sec_finalize_kernel, fgrid, fblock, 0, st, sa);
    KERNEL_TRY();
    for (int k = 1; k <= sa.n_sec && route == Route::Secondary; ++k) {
        DpArgs ta = a.da;
        ta.w_job = sa.s_job + static_cast<size_t>(k) * n;
        ta.w_end = sa.s_end + static_cast<size_t>(k) * n;
        ta.w_score = sa.s_score + static_cast<size_t>(k) * n;
        launch_pass2(c, route, ta, c->sec.d_sts.as<int32_t>() + 2 * static_cast<size_t>(k) * n, st);
        KERNEL_TRY();
    }
    sa.mode = 2;
    hipLaunchKernelGGL(sfa::sdtw_sec_finalize_kernel, fgrid, fblock, 0, st, sa);
    KERNEL_TRY();
    return SFA_OK;
}

// The batch on the context's stream: screen, row strips beside it, pass 1, pass 2, secondaries, the join and the error words;
// then its profile
int enqueue_batch(sfa_ctx *c, Route route, const BatchArgs &a, const sfa::LongPlan &lp) {
    hipStream_t st = c->stream;
    const DpArgs &da = a.da;
    int rc;
    if (da.prio_unit > 0) HIP_TRY(hipMemsetAsync(c->wave.d_started.p, 0, 4, st));
    HIP_TRY(hipEventRecord(c->ev[0], st));
    // reads with a NaN / inf query value are skipped (the reference aborts on them, see sdtw_screen_kernel)
    HIP_TRY(hipMemsetAsync(c->status.dev(), 0, sizeof(sfa::BatchStatus), st));
    hipLaunchKernelGGL(sfa::sdtw_screen_kernel, dim3((da.n_reads_total + 3) / 4), dim3(256), 0, st, da.queries, da.q_off, da.n_reads_total, c->status.d_bad.as<uint8_t>(),
                       &c->status.dev()->non_finite);
    KERNEL_TRY();
    // Queries beyond 2048 events: row strips, on their own stream BESIDE the wave kernels of the shorter reads of the batch (a
    // handful of short reads is one sweep's latency on an empty chip: 6 + 2.5 ms in front of 110 ms of strips when run in a
    // row).  The two paths write disjoint rows (the finalize kernels here leave the long reads' rows alone).
    if (!lp.reads.empty()) {
        hipStream_t ls = c->stream_long;
        HIP_TRY(hipEventRecord(c->lev[0], st));  // queries, offsets and the non-finite screen are ready
        HIP_TRY(hipStreamWaitEvent(ls, c->lev[0], 0));
        if ((rc = align_long(c, lp, da.queries, da.q_off, da.out, a.sa.sec, ls))) {
            (void)hipStreamSynchronize(ls);  // nothing of a failed call may still be running when the caller reuses its buffers
            (void)hipStreamSynchronize(c->stream_long2);
            return rc;
        }
        HIP_TRY(hipEventRecord(c->lev[1], ls));
    }
    if ((rc = enqueue_pass1(c, route, a, st))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], st));
    if ((rc = enqueue_pass2(c, route, a, st))) return rc;
    if (c->opt_secondary > 0 && (rc = enqueue_secondaries(c, route, a, st))) return rc;
    c->prof.fill_launches = (route != Route::NoQuads ? 1 : 0) + lp.n_groups;  // (a pass-1 launch per group of long reads)
    c->strips.long_pending = !lp.reads.empty();
    if (c->strips.long_pending) {  // join: what is left of the strips when the wave kernels are through counts as fill time
        HIP_TRY(hipEventRecord(c->ev[5], st));
        HIP_TRY(hipStreamWaitEvent(st, c->lev[1], 0));
        // the secondaries of the long reads, behind the join: every rank of every group has been traced, and the wave path's own
        // finalize, which wrote valid = 0 into these rows, is in front of this launch on this stream
        if (strip_secondaries(c) && a.sa.sec) {
            sfa::StripSecArgs xa = strip_sec_args(c, lp, 0, lp.n_long(), a.sa.sec);
            xa.mode = 2;
            hipLaunchKernelGGL(sfa::sdtw_strip_sec_finalize_kernel, dim3((xa.n_long + 63) / 64), dim3(64), 0, st, xa);
            KERNEL_TRY();
        }
    }
    HIP_TRY(hipMemcpyAsync(c->status.h_block.p, c->status.dev(), sizeof(sfa::BatchStatus), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(c->ev[4], st));

    const sfa::BatchPlan &plan = c->wave.plan;  // what resolve_profile() completes once the batch is through
    c->prof.cells = (plan.query_events + lp.events) * c->model.total_cols;
    c->prof.ckpt_interval = plan.ck_shift ? (1 << plan.ck_shift) : 0;
    c->prof.ckpt_bytes = static_cast<int64_t>(sizeof(float)) * plan.ck_floats;
    c->prof.lds_ckpt = route == Route::LdsFused ? 2 : (route == Route::Lds ? 1 : 0);
    c->prof.fused_trace = fused(route) ? 1 : 0;
    c->prof.trace_margin = plan.trace_margin;
    c->prof.n_tasks = plan.n_quads * plan.n_chunks;
    c->prof.n_chunks = plan.n_chunks;
    c->prof.n_segments = plan.n_seg;
    c->prof.segment_reruns = c->seg.seg_reruns;
    c->prof_pending = true;
    return SFA_OK;
}

}  // namespace

// Core of every align entry point: queries already in HBM, results left in HBM.
int sfa::align_device(sfa_ctx *c, const float *d_queries, const int64_t *q_off, int32_t n, ResultRow *d_out, ResultRow *d_sec) {
    if (!c->in_slice && !c->seg.no_segments_once) {  // the call sfa_event_maps refers to from now on (not: a slice or a re-run of it)
        c->maps.map_n = n;
        c->maps.map_q_off.assign(q_off, q_off + n + 1);
        c->maps.map_queries = d_queries;
    }
    if (n == 0) return SFA_OK;
    // secondary mappings: the plain two-pass route (HBM snapshots, no column segments, pass 2 as its own launches), whose fill keeps
    // every read's top-5 list; the candidates behind the primary are traced by the same pass-2 kernel, one launch per rank
    const int n_sec = static_cast<int>(c->opt_secondary);
    const bool own_sec = n_sec > 0 && !d_sec;  // the call's own secondaries: sec_n names them once they are all enqueued
    if (own_sec) {
        c->sec.sec_n = -1;  // a call that fails or returns early leaves no rows to be taken for its own
        if (int rc = c->sec.reserve_rows(static_cast<size_t>(n))) return rc;
        d_sec = c->sec.d_sec.as<ResultRow>();
    }
    // queries beyond the wave kernels' 2048 events: row strips, beside the rest of the batch
    const sfa::LongPlan lp = sfa::plan_long_reads(q_off, n, c->model.h_job_len, c->opt_ckpt_interval, c->opt_ckpt_budget, c->cu_count, c->opt_spin_limit_ms);
    sfa::PlanParams pp = plan_params(c);
    pp.skip_long = !lp.reads.empty();
    sfa::BatchPlan &plan = c->wave.plan;  // kept with the context: its vectors are reused by every batch
    std::string perr;
    if (int rc = sfa::plan_batch(q_off, n, c->model.h_job_len, c->model.total_cols, pp, &plan, &perr)) return fail(rc, "%s", perr.c_str());
    if (!c->in_slice && c->opt_ckpt_interval == 0 && plan.ck_shift > 9 && n >= 2 * c->opt_min_slice_reads) {
        // checkpoints at T = 512 would take about ck_bytes * T/512
        const int64_t want = (plan.ck_floats * 4 * (1ll << (plan.ck_shift - 9)) + pp.ckpt_budget_bytes - 1) / std::max<int64_t>(pp.ckpt_budget_bytes, 1);
        const int32_t slices = static_cast<int32_t>(std::min<int64_t>(want, n / c->opt_min_slice_reads));
        if (slices > 1) {
            const int rc = align_sliced(c, d_queries, q_off, n, d_out, d_sec, slices);
            if (!rc && own_sec) c->sec.sec_n = n;
            return rc;
        }
    }
    const Route route = sfa::choose_route(plan, pp.std_dtw, n_sec, c->opt_fused_trace, static_cast<int64_t>(c->cu_count) * 4 * SFA_LCK_WAVES);
    const Staging sg(n, plan, c->model.n_jobs);
    int rc;
    if ((rc = stage_and_reserve(c, q_off, n, route, sg))) return rc;
    HIP_TRY(hipMemcpyAsync(c->wave.d_stage.p, c->wave.h_stage.p, sg.bytes, hipMemcpyHostToDevice, c->stream));
    const BatchArgs a = batch_args(c, d_queries, n, d_out, d_sec, route, sg, !lp.reads.empty());
    if ((rc = enqueue_batch(c, route, a, lp))) return rc;
    if (route == Route::Segments) {
        // the verdict of the hand-over checks has to be known before anybody uses the rows: wait here (these are the small,
        // latency-bound batches -- their caller is about to wait for them anyway)
        int32_t *flags = c->seg.h_flags.as<int32_t>();
        HIP_TRY(hipMemcpyAsync(flags, c->seg.d_segfail.p, 4 * static_cast<size_t>(plan.n_quads), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (std::any_of(flags, flags + plan.n_quads, [](int32_t f) { return f != 0; })) {
            // a guessed state was not the true one somewhere: the batch is walked again, unsegmented
            c->seg.no_segments_once = true;
            rc = align_device(c, d_queries, q_off, n, d_out);
            c->seg.no_segments_once = false;
            c->seg.seg_reruns++;
            c->prof.segment_reruns = c->seg.seg_reruns;
            return rc;
        }
    }
    if (own_sec) c->sec.sec_n = n;
    return SFA_OK;
}

int sfa::resolve_profile(sfa_ctx *c) {
    if (!c->prof_pending) return SFA_OK;
    HIP_TRY(hipEventSynchronize(c->ev[4]));
    float a = 0, b = 0, d = 0, t = 0;
    HIP_TRY(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    HIP_TRY(hipEventElapsedTime(&d, c->ev[2], c->ev[3]));
    HIP_TRY(hipEventElapsedTime(&t, c->ev[0], c->ev[4]));
    if (c->prof.fused_trace) d = 0;  // pass 2 ran inside the fill launch: there was no trace launch to time
    if (c->strips.long_pending) {  // the row-strip sweeps of long queries are fills
        float l = 0;
        HIP_TRY(hipEventElapsedTime(&l, c->ev[5], c->ev[4]));
        a += l;
        a = t;  // ... and ran BESIDE the wave kernels: the intervals on this stream say nothing about stages
        d = 0;
        c->strips.long_pending = false;
    }
    c->prof.events_ms = c->prof.normalise_ms = 0;
    c->prof.decode_ms = 0;
    c->prof.blow5_fallbacks = c->blow5.blow5_fallbacks;
    if (c->blow5.bev_pending) {
        float d1 = 0;
        HIP_TRY(hipEventElapsedTime(&d1, c->bev[0], c->bev[1]));
        c->prof.decode_ms = d1;
        c->blow5.bev_pending = false;
    }
    if (c->raw.eev_pending) {
        float e1 = 0, e2 = 0;
        HIP_TRY(hipEventElapsedTime(&e1, c->eev[0], c->eev[1]));
        HIP_TRY(hipEventElapsedTime(&e2, c->eev[2], c->eev[3]));
        c->prof.events_ms = e1;
        c->prof.normalise_ms = e2;
        c->raw.eev_pending = false;
    }
    const sfa::BatchStatus *bs = c->status.host();  // (copied before ev[4], which has been waited for)
    c->prof.non_finite_reads = bs ? bs->non_finite : 0;
    c->prof.lck_fallbacks = bs ? bs->lck_fallbacks : 0;
    c->prof.lck_from_scratch = bs ? bs->lck_from_scratch : 0;
    c->prof.fill_ms = a;
    c->prof.trace_ms = d;
    c->prof.finalize_ms = t - a - d;
    c->prof.total_ms = t;
    c->prof_pending = false;
    if (!bs) return SFA_OK;
    const unsigned *e = bs->err;  // a wave of the batch gave up waiting for another one (bounded_wait_ge): the rows are not to be used
    if (e[0] == sfa::kErrQuadWait)
        return fail(SFA_EKERNEL, "fused launch: pass 2 of quad %u waited %lld ms for its fill tasks (%u of them had completed); rows of this batch are invalid",
                    e[1], (long long)c->wave.quad_limit_ms, e[2]);
    if (e[0] == sfa::kErrStripWait)
        return fail(SFA_EKERNEL, "row strips: a strip waited %lld ms for column %u of the row above (column %u was published); rows of this batch are invalid",
                    (long long)c->strips.strip_limit_ms, e[1], e[2]);
    if (e[0]) return fail(SFA_EKERNEL, "device error word %u (%u, %u)", e[0], e[1], e[2]);
    // spans of this (valid) batch's alignments -> head start of the next batch's pass 2 (sfa_plan.hpp)
    const unsigned *h = bs->span_hist;
    uint64_t total = 0;
    for (int b = 0; b < sfa::kSpanBuckets; ++b) total += h[b];
    if (total >= 64) {  // the bucket below which 99.9 % of the alignments lie (its upper edge: b + 1 sixteenths) and one more, never above a whole query
        uint64_t acc = 0;
        int b = 0;
        for (; b < sfa::kSpanBuckets; ++b) {
            acc += h[b];
            if (acc * 1000 >= total * 999) break;
        }
        c->wave.span_sixteenths = std::min(16, b + 2);
    }
    return SFA_OK;
}

extern "C" {

int sfa_align_batch_device(sfa_ctx_t *c, const float *d_queries, const int64_t *q_off, int32_t n, sfa_result_t *d_out, int sync) {
    if (!c || !q_off || n < 0 || (n > 0 && (!d_queries || !d_out))) return fail(SFA_EINVAL, "sfa_align_batch_device: bad argument");
    if (!c->shards.empty())
        return fail(SFA_EINVAL, "sfa_align_batch_device: device-resident buffers belong to one device; use a single-device context "
                                "(sfa_init) per GPU, or the host-buffer entry points on a group context");
    HIP_TRY(hipSetDevice(c->device));
    // the pinned staging area is reused by every call: the previous batch must have left it
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = resolve_profile(c)) return rc;
    if (int rc = align_device(c, d_queries, q_off, n, reinterpret_cast<ResultRow *>(d_out))) return rc;
    if (sync) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return resolve_profile(c);
    }
    return SFA_OK;
}

int sfa_submit_batch(sfa_ctx_t *c, const float *queries, const int64_t *q_off, int32_t n) {
    if (!c || !q_off || n < 0 || (n > 0 && !queries)) return fail(SFA_EINVAL, "sfa_submit_batch: bad argument");
    if (!c->shards.empty()) {  // every shard queues its contiguous range of reads on its own device
        c->io.pending_n = -1;
        const int rc = for_each_shard_range(c, n, [&](size_t r, int32_t lo, int32_t hi) {
            return sfa_submit_batch(c->shards[r], queries, q_off + lo, hi - lo);  // (q_off holds absolute offsets into queries)
        }, &c->shard_lo);  // (sfa_wait_batch collects by the same ranges)
        if (!rc) c->io.pending_n = n;
        c->maps.map_n = rc ? -1 : n;
        return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // one batch in flight per context
    if (int rc = resolve_profile(c)) return rc;  // a batch submitted and never waited for: its error words are this call's
    c->io.pending_n = -1;
    if (n == 0) {
        c->io.pending_n = 0;
        return SFA_OK;
    }
    const int64_t nq = q_off[n] - q_off[0];
    if (nq < 0) return fail(SFA_EINVAL, "q_off not monotone");
    int rc;
    // the device path indexes queries by q_off directly, so upload the span [q_off[0], q_off[n]) re-based to 0
    std::vector<int64_t> rebased;
    const int64_t *qo = q_off;
    if (q_off[0] != 0) {
        rebased.resize(n + 1);
        for (int32_t i = 0; i <= n; ++i) rebased[i] = q_off[i] - q_off[0];
        qo = rebased.data();
    }
    if ((rc = c->io.reserve(nq, static_cast<size_t>(n)))) return rc;
    HIP_TRY(hipMemcpyAsync(c->io.d_queries.p, queries + q_off[0], sizeof(float) * nq, hipMemcpyHostToDevice, c->stream));
    if ((rc = align_device(c, c->io.d_queries.as<float>(), qo, n, c->io.d_out.as<ResultRow>()))) return rc;
    HIP_TRY(hipMemcpyAsync(c->io.h_out.p, c->io.d_out.p, sizeof(sfa_result_t) * n, hipMemcpyDeviceToHost, c->stream));
    c->io.pending_n = n;
    return SFA_OK;
}

int sfa_wait_batch(sfa_ctx_t *c, sfa_result_t *out, int32_t n) {
    if (!c || n < 0 || (n > 0 && !out)) return fail(SFA_EINVAL, "sfa_wait_batch: bad argument");
    if (c->io.pending_n < 0) return fail(SFA_EINVAL, "sfa_wait_batch: no batch was submitted");
    if (c->io.pending_n != n) return fail(SFA_EINVAL, "sfa_wait_batch: %d reads were submitted, %d asked for", c->io.pending_n, n);
    c->io.pending_n = -1;
    if (!c->shards.empty())  // rows of shard r go to out[lo_r, hi_r): input order, no gather step in a single process
        return for_each_shard(c, [&](size_t r) {  // (shards without reads were not submitted to)
            const int32_t lo = c->shard_lo[r], hi = c->shard_lo[r + 1];
            return lo == hi ? static_cast<int>(SFA_OK) : sfa_wait_batch(c->shards[r], out + lo, hi - lo);
        });
    if (n == 0) return SFA_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, c->io.h_out.p, sizeof(sfa_result_t) * n);
    return resolve_profile(c);
}

int sfa_secondary_rows(sfa_ctx_t *c, sfa_result_t *sec, int32_t n) {
    if (!c || n < 0 || (n > 0 && !sec)) return fail(SFA_EINVAL, "sfa_secondary_rows: bad argument");
    if (!c->shards.empty()) {  // every entry point splits a call the same way (shard_ranges): shard r holds rows [lo_r, hi_r)
        if (c->shards[0]->opt_secondary == 0) return fail(SFA_EINVAL, "sfa_secondary_rows: the 'secondary' option is 0");
        return for_each_shard_range(c, n, [&](size_t r, int32_t lo, int32_t hi) {
            return sfa_secondary_rows(c->shards[r], sec + 4 * static_cast<size_t>(lo), hi - lo);
        });
    }
    if (c->opt_secondary == 0) return fail(SFA_EINVAL, "sfa_secondary_rows: the 'secondary' option is 0");
    if (n == 0) return SFA_OK;
    if (c->sec.sec_n != n) return fail(SFA_EINVAL, "sfa_secondary_rows: the last call aligned %d reads with secondaries, %d asked for", c->sec.sec_n, n);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(sec, c->sec.d_sec.p, 4 * sizeof(sfa_result_t) * static_cast<size_t>(n), hipMemcpyDeviceToHost));
    return SFA_OK;
}

int sfa_align_batch(sfa_ctx_t *c, const float *queries, const int64_t *q_off, int32_t n, sfa_result_t *out) {
    if (!c || !q_off || n < 0 || (n > 0 && (!queries || !out))) return fail(SFA_EINVAL, "sfa_align_batch: bad argument");
    if (int rc = sfa_submit_batch(c, queries, q_off, n)) return rc;
    return sfa_wait_batch(c, out, n);
}

int sfa_align_events(sfa_ctx_t *c, const sfa_event_t *const *events, const int64_t *n_events, const int64_t *qstart,
                     const int64_t *qend, int32_t n, sfa_result_t *out) {
    if (!c || n < 0 || (n > 0 && (!events || !n_events || !qstart || !qend || !out)))
        return fail(SFA_EINVAL, "sfa_align_events: bad argument");
    // gather db->et[i].event[qstart..qend).mean (AoS, stride 24 B) into the packed SoA the kernels read
    std::vector<int64_t> q_off(n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        int64_t l = 0;
        if (n_events[i] > 0 && events[i]) {
            if (qstart[i] < 0 || qend[i] < qstart[i] || qend[i] > n_events[i])
                return fail(SFA_EINVAL, "sfa_align_events: read %d has query window [%lld,%lld) outside its %lld events", i,
                            (long long)qstart[i], (long long)qend[i], (long long)n_events[i]);
            l = qend[i] - qstart[i];
        }
        q_off[i + 1] = q_off[i] + l;
    }
    // the gather reads 24 bytes per event to keep 4: a 100 000-read batch is 600 MB through one core (70-90 ms, as long as
    // the whole alignment) unless it is spread over a few threads; a single-device context gathers straight into page-locked
    // memory, from where the upload is a true asynchronous copy
    const int64_t total = q_off[n];
    float *dst = nullptr;
    std::unique_ptr<float[]> heap;
    if (c->shards.empty()) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // the previous batch may still be uploading from the buffer
        if (int rc = c->io.h_queries.reserve(sizeof(float) * static_cast<size_t>(std::max<int64_t>(total, 1)))) return rc;
        dst = c->io.h_queries.as<float>();
    } else {
        heap.reset(new float[static_cast<size_t>(std::max<int64_t>(total, 1))]);
        dst = heap.get();
    }
    auto gather = [&](int32_t lo, int32_t hi) {
        for (int32_t i = lo; i < hi; ++i) {
            const int64_t l = q_off[i + 1] - q_off[i];
            const sfa_event_t *ev = l ? events[i] + qstart[i] : nullptr;
            float *d = dst + q_off[i];
            for (int64_t j = 0; j < l; ++j) d[j] = ev[j].mean;
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int n_thr = total < (int64_t(1) << 21) ? 1 : static_cast<int>(std::min<int64_t>(std::min(8u, hw), total >> 20));
    if (n_thr <= 1) {
        gather(0, n);
    } else {  // contiguous read ranges of about equal event counts
        std::vector<std::thread> th;
        int32_t lo = 0;
        for (int t = 0; t < n_thr; ++t) {
            const int64_t want = total * (t + 1) / n_thr;
            int32_t hi = (t + 1 == n_thr) ? n : static_cast<int32_t>(std::upper_bound(q_off.begin() + lo, q_off.begin() + n + 1, want) - q_off.begin() - 1);
            hi = std::max(hi, lo);
            if (t + 1 == n_thr)
                gather(lo, hi);
            else
                th.emplace_back(gather, lo, hi);
            lo = hi;
        }
        for (std::thread &x : th) x.join();
    }
    return sfa_align_batch(c, dst, q_off.data(), n, out);
}

}  // extern "C"
