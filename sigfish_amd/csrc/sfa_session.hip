// sfa_session.hip -- alignment sessions of the C-ABI (include/sigfish_amd.h): a slot's subsequence DTW extended chunk by chunk
// (sdtw_session.hpp).  A session belongs to its context, runs on the context's stream and is freed with it at the latest.  Its
// state is one struct per feature (namespace sess, sfa_session_state.hpp, which lists them).  This unit holds creation, the sweep
// behind both extend entry points, raw mode, the event maps and the spread sessions; targets, groups, caps, reach lists and the
// query calls that read a slot's carried row are sfa_session_targets.hip's.
#define SFA_DEFINE_SESSION_KERNELS  // (this unit holds the plain kernels of sdtw_session.hpp and events_stream.hpp)
#include "sfa_session_state.hpp"
#include "events_auto_stream.hpp"

namespace sfa {
// defined in sfa_align.hip, the unit that holds the plain kernels of sdtw_kernels.hpp
__global__ void sdtw_screen_kernel(const float *queries, const int64_t *q_off, const int n, uint8_t *bad, unsigned *count);
}  // namespace sfa

namespace {

const sfa_result_t kNoRow = sfa::to_result(sfa::no_row());
size_t align8(size_t x) { return (x + 7) & ~static_cast<size_t>(7); }
constexpr uint32_t kSessionFlags = SFA_SESSION_NO_START | SFA_SESSION_RESWEEP | SFA_SESSION_SPREAD;  // (0x2 is not assigned)

// the number the caller knows slot sl by (a sub-session of a spread session holds every G-th slot)
int32_t slot_name(const sfa_session *s, int32_t sl) { return sl * s->name_step + s->name_first; }

// the first slot that is not empty (events, a poison flag, or samples in raw mode), -1: every slot is
int32_t first_busy_slot(const sfa_session *s) {
    for (int32_t sl = 0; sl < s->n_slots; ++sl)
        if (s->rows.len[sl] != 0 || s->rows.poison[sl] || (s->raw.on && !s->raw.slots[sl].fresh)) return sl;
    return -1;
}

// (a slot's next chunk is a first chunk: nothing of its carried row is read)
void reset_slot(sfa_session *s, int32_t sl) {
    s->rows.len[sl] = 0;
    s->rows.poison[sl] = 0;
    if (s->raw.on) s->raw.reset_slot(sl);
    if (s->autos.on()) s->autos.reset_slot(sl);
}

// the sweep kernel of the session's kind (with candidates every piece of a long chunk keeps a list: the last one's stays)
void launch_sweep_kernel(const sfa_session *s, hipStream_t st, const sfa::SessionArgs &a) {
    auto *kernel = s->cand.n_cand > 0 ? (s->track ? sfa::sdtw_session_kernel<true, true> : sfa::sdtw_session_kernel<false, true>)
                                      : (s->track ? sfa::sdtw_session_kernel<true> : sfa::sdtw_session_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3((a.n_tasks + 3) / 4), dim3(256), 0, st, a);
}

// ---- the sweep, the core of both extend entry points: plan -> stage -> launch -> collect ----
// Chunk i of the call, ch[i], is swept below the carried row of slot[i].  d_events == nullptr ("screen"): the chunks are the nq
// host floats behind h_events (may be NULL when nq is 0), back to back; they are uploaded and screened for NaN / inf here.  Else
// they lie in d_events already (offsets of any kind), and sweep.d_bad holds the call's poison flags.

// staging: [chunk offsets (n + 1) x i64 | call_slot n x i32 | per launch: k_off i64, w_entry, g_qlen, k_call, k_slot, k_len, k_total]
// and, on a session that keeps its events, behind all that: [slot n x i32 | events the slot had n x i32]
size_t sweep_cslot_at(int32_t n) { return align8(8 * static_cast<size_t>(n + 1)); }

int sweep_stage(sfa_session *s, const int32_t *slot, const sfa::Chunk *ch, int32_t n, int64_t nq, const float *d_events) {
    sfa_ctx *c = s->c;
    sess::Sweep &w = s->sweep;
    size_t bytes = sweep_cslot_at(n) + align8(4 * static_cast<size_t>(n));
    for (const sfa::Launch &l : w.launches) bytes += 8 * l.k_off.size() + align8(4 * (l.w_entry.size() + l.g_qlen.size() + 4 * l.k_off.size()));
    const bool keep = s->keep.on() && !d_events;
    if (keep) bytes += 2 * align8(4 * static_cast<size_t>(n));
    const size_t n_part = static_cast<size_t>(n) * c->model.n_jobs;
    if (int rc = w.reserve(bytes, nq, static_cast<size_t>(n), n_part)) return rc;
    if (int rc = s->cand.reserve_call(n_part)) return rc;
    char *h = w.h_stage.as<char>();
    const char *d = w.d_stage.as<char>();
    for (int32_t i = 0; i < n; ++i) reinterpret_cast<int64_t *>(h)[i] = ch[i].off;  // (read by the screen only)
    reinterpret_cast<int64_t *>(h)[n] = nq;
    memcpy(h + sweep_cslot_at(n), w.call_slot.data(), 4 * static_cast<size_t>(n));
    size_t at = sweep_cslot_at(n) + align8(4 * static_cast<size_t>(n));
    auto put = [&](const void *src, size_t nbytes) {  // at the next free byte of the staging; its offset
        const size_t here = at;
        if (nbytes) memcpy(h + at, src, nbytes);
        at = here + nbytes;
        return here;
    };
    w.args.resize(w.launches.size());
    for (size_t li = 0; li < w.launches.size(); ++li) {
        const sfa::Launch &l = w.launches[li];
        const size_t m = l.k_off.size();
        sfa::SessionArgs &a = w.args[li];
        memset(&a, 0, sizeof a);
        a.k_off = reinterpret_cast<const int64_t *>(d + put(l.k_off.data(), 8 * m));
        a.w_entry = reinterpret_cast<const int32_t *>(d + put(l.w_entry.data(), 4 * l.w_entry.size()));
        a.g_qlen = reinterpret_cast<const int32_t *>(d + put(l.g_qlen.data(), 4 * l.g_qlen.size()));
        a.k_call = reinterpret_cast<const int32_t *>(d + put(l.k_call.data(), 4 * m));
        a.k_slot = reinterpret_cast<const int32_t *>(d + put(l.k_slot.data(), 4 * m));
        a.k_len = reinterpret_cast<const int32_t *>(d + put(l.k_len.data(), 4 * m));
        a.k_total = reinterpret_cast<const int32_t *>(d + put(l.k_total.data(), 4 * m));
        at = align8(at);
        a.events = d_events ? d_events : w.d_events.as<float>();
        a.bad = w.d_bad.as<uint8_t>();
        a.ref = c->model.d_ref.as<float>();
        a.job_off = c->model.d_job_off.as<int64_t>();
        a.job_len = c->model.d_job_len.as<int32_t>();
        a.col_off = s->rows.d_col_off.as<int64_t>();
        a.row_c = s->rows.d_row_c.as<float>();
        a.row_s = s->track ? s->rows.d_row_s.as<int32_t>() : nullptr;
        a.row_stride = c->model.total_cols;
        a.p_best = w.d_pbest.as<float>();
        a.p_second = w.d_psecond.as<float>();
        a.p_end = w.d_pend.as<int32_t>();
        a.p_st = w.d_pst.as<int32_t>();
        for (int ci = 0; ci < l.n_cls; ++ci) a.cls[ci] = l.cls[ci];
        a.n_cls = l.n_cls;
        a.n_jobs = c->model.n_jobs;
        a.n_tasks = l.n_tasks;
        a.p_top5 = s->cand.n_cand > 0 ? s->cand.d_p5.as<int32_t>() : nullptr;
    }
    w.keep_at = 0;
    if (keep) {  // (rows.len is still what the slots held before this call: sweep_collect adds the chunks)
        w.keep_at = at;
        int32_t *ks = reinterpret_cast<int32_t *>(h + at), *kh = reinterpret_cast<int32_t *>(h + at + align8(4 * static_cast<size_t>(n)));
        for (int32_t i = 0; i < n; ++i) ks[i] = slot[i], kh[i] = static_cast<int32_t>(s->rows.len[slot[i]]);
        at += 2 * align8(4 * static_cast<size_t>(n));
    }
    if (at > bytes) return fail(SFA_EKERNEL, "session sweep: staging overrun (%zu > %zu)", at, bytes);
    w.staged = at;
    return SFA_OK;
}

int sweep_launch(sfa_session *s, int32_t n, const float *h_events, int64_t nq, bool screen) {
    sfa_ctx *c = s->c;
    sess::Sweep &w = s->sweep;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(w.d_stage.p, w.h_stage.p, w.staged, hipMemcpyHostToDevice, st));
    if (screen && nq > 0) HIP_TRY(hipMemcpyAsync(w.d_events.p, h_events, sizeof(float) * nq, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.d_count.p, 0, 4, st));
    HIP_TRY(hipEventRecord(w.ev[0], st));
    if (w.keep_at) {  // a session that keeps its events: the chunks into the slots' kept events, in front of the sweep
        sfa::SessionKeepArgs ka;
        ka.events = w.d_events.as<float>();
        ka.ch_off = w.d_stage.as<int64_t>();
        ka.slot = reinterpret_cast<const int32_t *>(w.d_stage.as<char>() + w.keep_at);
        ka.have = reinterpret_cast<const int32_t *>(w.d_stage.as<char>() + w.keep_at + align8(4 * static_cast<size_t>(n)));
        ka.keep = s->keep.d_keep.as<float>();
        ka.over = s->keep.d_over.as<uint8_t>();
        ka.n = n;
        ka.max_events = s->keep.max_events;
        hipLaunchKernelGGL(sfa::sdtw_session_keep_kernel, dim3(n), dim3(256), 0, st, ka);
        KERNEL_TRY();
    }
    // chunks with a NaN / inf event are not swept: the slot is poisoned (rows valid = 0 until reset)
    if (screen) {
        hipLaunchKernelGGL(sfa::sdtw_screen_kernel, dim3((n + 3) / 4), dim3(256), 0, st, w.d_events.as<float>(), w.d_stage.as<int64_t>(), n, w.d_bad.as<uint8_t>(),
                           w.d_count.as<unsigned>());
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(w.ev[1], st));
    for (const sfa::SessionArgs &a : w.args) {
        launch_sweep_kernel(s, st, a);
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(w.ev[2], st));
    sfa::SessionRowsArgs ra;  // the rows of the call's slots from the partial results, and their candidates
    ra.call_slot = reinterpret_cast<const int32_t *>(w.d_stage.as<char>() + sweep_cslot_at(n));
    ra.bad = w.d_bad.as<uint8_t>();
    ra.p_best = w.d_pbest.as<float>();
    ra.p_second = w.d_psecond.as<float>();
    ra.p_end = w.d_pend.as<int32_t>();
    ra.p_st = w.d_pst.as<int32_t>();
    ra.ref = c->model.tables();
    ra.rows = s->rows.d_rows.as<sfa::ResultRow>();
    ra.n_call = n;
    ra.n_jobs = c->model.n_jobs;
    ra.track = s->track ? 1 : 0;
    hipLaunchKernelGGL(sfa::sdtw_session_rows_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ra);
    KERNEL_TRY();
    if (s->cand.n_cand > 0 && !w.args.empty()) {  // (nothing swept: every slot keeps its candidates)
        sfa::SessionCandArgs ca;
        ca.call_slot = ra.call_slot;
        ca.bad = ra.bad;
        ca.p_top5 = s->cand.d_p5.as<int32_t>();
        ca.ref = ra.ref;
        ca.cand = s->cand.d_cand.as<sfa::ResultRow>();
        ca.n_call = n;
        ca.n_jobs = ra.n_jobs;
        ca.n_cand = s->cand.n_cand;
        ca.track = ra.track;
        hipLaunchKernelGGL(sfa::sdtw_session_cand_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ca);
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(w.ev[3], st));
    HIP_TRY(hipMemcpyAsync(s->rows.h_rows.p, s->rows.d_rows.p, sizeof(sfa_result_t) * s->n_slots, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(w.h_bad.p, w.d_bad.p, static_cast<size_t>(n), hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "session sweep: the launches failed: %s", hipGetErrorString(hipGetLastError()));
    return SFA_OK;
}

// lengths, poison flags, the caller's rows, the context's profile
int sweep_collect(sfa_session *s, const int32_t *slot, const sfa::Chunk *ch, int32_t n, int64_t new_events, sfa_result_t *out) {
    sfa_ctx *c = s->c;
    const uint8_t *bad = s->sweep.h_bad.as<uint8_t>();
    const sfa_result_t *rows = s->rows.h_rows.as<sfa_result_t>();
    int64_t non_finite = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        s->rows.len[sl] += ch[i].len;
        if (bad[i]) s->rows.poison[sl] = 1;
        non_finite += s->rows.poison[sl];
        out[i] = (s->rows.poison[sl] || s->rows.len[sl] == 0) ? kNoRow : rows[sl];
    }
    float t_fill = 0, t_total = 0;
    HIP_TRY(hipEventElapsedTime(&t_fill, s->sweep.ev[1], s->sweep.ev[2]));
    HIP_TRY(hipEventElapsedTime(&t_total, s->sweep.ev[0], s->sweep.ev[3]));
    sfa_profile_t pr{};
    pr.fill_ms = t_fill;
    pr.total_ms = t_total;
    pr.finalize_ms = t_total - t_fill;
    pr.cells = new_events * c->model.total_cols;
    pr.fill_launches = static_cast<int64_t>(s->sweep.args.size());
    for (const sfa::SessionArgs &a : s->sweep.args) pr.n_tasks += a.n_tasks;
    pr.n_chunks = c->model.n_jobs;
    pr.n_segments = 1;
    pr.non_finite_reads = non_finite;
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    c->prof = pr;
    return SFA_OK;
}

int sweep_chunks(sfa_session *s, const int32_t *slot, const sfa::Chunk *ch, int32_t n, const float *h_events, int64_t nq, const float *d_events, sfa_result_t *out) {
    int64_t new_events = 0;
    sfa::plan_session_call(ch, slot, s->rows.len.data(), s->rows.poison.data(), n, s->c->model.n_jobs, &s->sweep.launches, &s->sweep.call_slot, &new_events);
    if (int rc = sweep_stage(s, slot, ch, n, nq, d_events)) return rc;
    if (int rc = sweep_launch(s, n, h_events, nq, d_events == nullptr)) return rc;
    return sweep_collect(s, slot, ch, n, new_events, out);
}

// ---- sfa_session_extend_raw, stage by stage (what a stage hands on lies in sess::Raw / sess::AutoStart, "of a call") ----

int raw_check(sfa_session *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n) {
    sess::Raw &r = s->raw;
    begin_call(s);
    r.scale.resize(2 * static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        if (int rc = claim_slot(s, sl, "sfa_session_extend_raw")) return rc;
        const int64_t l = raw_off[i + 1] - raw_off[i];
        if (l < 0) return fail(SFA_EINVAL, "sfa_session_extend_raw: raw_off not monotone");
        if (l > 0 && (r.slots[sl].status & sfa::kRawEnded)) return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d has seen its end of read; it takes no samples until it is reset", slot_name(s, sl));
        if (r.slots[sl].n + l > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_extend_raw: slot %d would hold more than 2^30 samples", slot_name(s, sl));
        const double *sc = scaling + 3 * static_cast<size_t>(i);
        if (!r.slots[sl].fresh && memcmp(sc, r.slots[sl].scaling, 3 * sizeof(double)) != 0)
            return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d: digitisation, offset and range are fixed by a slot's first chunk after a reset", slot_name(s, sl));
        const sfa::RawScale rs = sfa::raw_scale(sc[0], sc[1], sc[2]);
        r.scale[2 * static_cast<size_t>(i)] = rs.offset;
        r.scale[2 * static_cast<size_t>(i) + 1] = rs.unit;
        if (!std::isfinite(rs.offset) || !std::isfinite(rs.unit)) return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d: the scaling is not finite", slot_name(s, sl));
    }
    const int64_t total = raw_off[n] - raw_off[0];
    if (total > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_extend_raw: more than 2^30 samples in one call");
    if (total > 0 && !raw) return fail(SFA_EINVAL, "sfa_session_extend_raw: null samples");
    return SFA_OK;
}

// entry tables: [raw_off re-based (n + 1) x i64 | slot n x i32 | flags n x i32 | scale 2n x f32], and with the automatic query
// start | have n x i32 | EvAutoEntry n.  The detector's argument block takes their device addresses; the other kernels copy them
int raw_stage_tables(sfa_session *s, const int32_t *slot, const int64_t *raw_off, const uint8_t *end_of_read, int32_t n) {
    sess::Raw &r = s->raw;
    const size_t nn = static_cast<size_t>(n), o_slot = align8(8 * (nn + 1)), o_flag = o_slot + align8(4 * nn), o_scale = o_flag + align8(4 * nn);
    r.o_have = o_scale + 8 * nn, r.o_aent = r.o_have + align8(4 * nn);
    r.staged = s->autos.on() ? r.o_aent + sizeof(sfa::EvAutoEntry) * nn : r.o_have;
    if (int rc = r.reserve_call(r.staged, raw_off[n] - raw_off[0], nn)) return rc;
    if (int rc = s->sweep.reserve_bad(nn)) return rc;  // (the normalisation writes the call's poison flags, the sweep reads them)
    char *h = r.h_rstage.as<char>();
    const char *d = r.d_rstage.as<char>();
    for (int32_t i = 0; i <= n; ++i) reinterpret_cast<int64_t *>(h)[i] = raw_off[i] - raw_off[0];
    for (int32_t i = 0; i < n; ++i) {
        reinterpret_cast<int32_t *>(h + o_slot)[i] = slot[i];
        reinterpret_cast<int32_t *>(h + o_flag)[i] = (r.slots[slot[i]].fresh ? sfa::kEntryFresh : 0) | ((end_of_read && end_of_read[i]) ? sfa::kEntryEnd : 0);
    }
    memcpy(h + o_scale, r.scale.data(), 8 * nn);
    r.ea.raw_off = reinterpret_cast<const int64_t *>(d);
    r.ea.slot = reinterpret_cast<const int32_t *>(d + o_slot);
    r.ea.e_flags = reinterpret_cast<const int32_t *>(d + o_flag);
    r.ea.scale = reinterpret_cast<const float *>(d + o_scale);
    return SFA_OK;
}

// automatic query start: the points this call carries every slot past (session_plan.hpp: auto_points)
int raw_plan_points(sfa_session *s, const int32_t *slot, const int64_t *raw_off, const uint8_t *end_of_read, int32_t n) {
    sess::AutoStart &au = s->autos;
    if (!au.on()) return SFA_OK;
    char *h = s->raw.h_rstage.as<char>();
    au.n_pending = 0;
    for (int32_t i = 0; i < n; ++i) {
        const sess::Raw::Slot &x = s->raw.slots[slot[i]];
        const sess::AutoStart::Slot &y = au.slots[slot[i]];
        reinterpret_cast<int32_t *>(h + s->raw.o_have)[i] = static_cast<int32_t>(x.n);
        const bool ended_now = end_of_read && end_of_read[i] && !(x.status & sfa::kRawEnded);
        const sfa::AutoPoints p = au.call[i] = sfa::auto_points(x.n, x.n + (raw_off[i + 1] - raw_off[i]), ended_now, au.every, au.max_samples, y.k, y.h.target >= 0 || y.final_taken);
        if (p.pending) reinterpret_cast<sfa::EvAutoEntry *>(h + s->raw.o_aent)[au.n_pending++] = sfa::EvAutoEntry{i, p.n0, p.n_periodic, p.n_final};
    }
    return au.reserve_call(au.n_pending, static_cast<size_t>(n));
}

int raw_launch_detector(sfa_session *s, const int16_t *raw, const int64_t *raw_off, int32_t n) {
    sess::Raw &r = s->raw;
    hipStream_t st = s->c->stream;
    const int64_t total = raw_off[n] - raw_off[0];
    HIP_TRY(hipMemcpyAsync(r.d_rstage.p, r.h_rstage.p, r.staged, hipMemcpyHostToDevice, st));
    if (total > 0) HIP_TRY(hipMemcpyAsync(r.d_raw.p, raw + raw_off[0], 2 * static_cast<size_t>(total), hipMemcpyHostToDevice, st));
    const sfa::DetectorParams dp = sfa::detector_params((s->c->flag & SFA_RNA) != 0);
    sfa::EvStreamArgs &ea = r.ea;
    ea.raw = r.d_raw.as<int16_t>();
    ea.state = r.d_state.as<sfa::EvStreamSlot>();
    ea.events = r.d_evtab.as<sfa::EvRecord>();
    ea.n = n;
    ea.ev_cap = r.ev_cap();
    ea.w1 = dp.w1, ea.w2 = dp.w2;
    ea.thr1 = dp.thr1, ea.thr2 = dp.thr2, ea.peak_height = dp.peak_height;
    HIP_TRY(hipEventRecord(r.ev_raw[0], st));
    hipLaunchKernelGGL(sfa::ev_stream_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ea);
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(r.ev_raw[1], st));
    return SFA_OK;
}

// automatic query start: the chunks into the retention buffers, then the points (slots without a pending point cost nothing)
int raw_launch_auto(sfa_session *s, int32_t n) {
    sess::AutoStart &au = s->autos;
    if (!au.on()) return SFA_OK;
    const sfa::EvStreamArgs &ea = s->raw.ea;
    hipStream_t st = s->c->stream;
    const char *d = s->raw.d_rstage.as<char>();
    sfa::EvAutoAppendArgs ap;
    ap.raw = ea.raw;
    ap.raw_off = ea.raw_off;
    ap.slot = ea.slot;
    ap.e_flags = ea.e_flags;
    ap.have = reinterpret_cast<const int32_t *>(d + s->raw.o_have);
    ap.keep = au.d_keep.as<int16_t>();
    ap.state = au.d_auto.as<sfa::EvAutoSlot>();
    ap.n = n;
    ap.max_samples = au.max_samples;
    HIP_TRY(hipEventRecord(au.ev_auto[0], st));
    hipLaunchKernelGGL(sfa::ev_auto_append_kernel, dim3(n), dim3(256), 0, st, ap);
    KERNEL_TRY();
    if (au.n_pending > 0) {
        sfa::EvAutoEvalArgs va;
        va.entries = reinterpret_cast<const sfa::EvAutoEntry *>(d + s->raw.o_aent);
        va.slot = ea.slot;
        va.scale = ea.scale;
        va.keep = ap.keep;
        va.csum = au.d_csum.as<int32_t>();
        va.state = ap.state;
        va.n_entries = au.n_pending;
        va.max_samples = au.max_samples;
        va.every = au.every;
        va.lo = sfa::adaptor_params(s->c->pore).lo;
        va.std_scale = sfa::adaptor_params(s->c->pore).std_scale;
        hipLaunchKernelGGL(sfa::ev_auto_eval_kernel, dim3(au.n_pending), dim3(64), 0, st, va);
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(au.ev_auto[1], st));
    return SFA_OK;
}

// the normalisation, and the wait for the call's counts of new events: the planner of the sweep is host code
int raw_launch_norm(sfa_session *s, int32_t n) {
    sfa_ctx *c = s->c;
    hipStream_t st = c->stream;
    const sess::Raw &r = s->raw;
    const sess::AutoStart &au = s->autos;
    sfa::EvNormArgs na;
    na.slot = r.ea.slot;
    na.state = r.ea.state;
    na.window = r.d_window.as<int32_t>();
    na.events = r.ea.events;
    na.query = r.d_query.as<float>();
    na.out = r.d_rout.as<sfa::EvStreamOut>();
    na.bad = s->sweep.d_bad.as<uint8_t>();
    na.n = n;
    na.ev_cap = r.ea.ev_cap;
    na.skip = r.skip;
    na.norm = r.norm;
    na.query_cap = r.query;
    na.n_at = r.recal_n;
    na.flags = r.recal_flags;
    for (int32_t j = 0; j < sfa::kRecalMaxPoints; ++j) na.at[j] = j < r.recal_n ? r.recal_at[j] : 0;
    na.resweep = s->resweep ? 1 : 0;
    na.reversed = (s->resweep && (c->flag & SFA_RNA) && !(c->flag & SFA_INV)) ? 1 : 0;
    if (au.on()) {
        const sfa::EvNormAutoArgs nx{au.d_auto.as<sfa::EvAutoSlot>(), au.d_aout.as<sfa::EvAutoSlot>()};
        hipLaunchKernelGGL(sfa::ev_stream_norm_kernel<true>, dim3(n), dim3(64), 0, st, na, nx);
        HIP_TRY(hipMemcpyAsync(au.h_aout.p, au.d_aout.p, sizeof(sfa::EvAutoSlot) * n, hipMemcpyDeviceToHost, st));
    } else {
        hipLaunchKernelGGL(sfa::ev_stream_norm_kernel<false>, dim3(n), dim3(64), 0, st, na, sfa::EvNormAutoArgs());  // (two null pointers)
    }
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(r.ev_raw[2], st));
    HIP_TRY(hipMemcpyAsync(r.h_rout.p, r.d_rout.p, sizeof(sfa::EvStreamOut) * n, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "sfa_session_extend_raw: the detector failed: %s", hipGetErrorString(hipGetLastError()));
    return SFA_OK;
}

// what the call left in every slot it named, and the chunks of new query events the sweep takes
void raw_take_results(sfa_session *s, const int32_t *slot, const int64_t *raw_off, const double *scaling, int32_t n, sfa::Chunk *ch) {
    sess::Raw &r = s->raw;
    sess::AutoStart &au = s->autos;
    const sfa::EvStreamOut *ro = r.h_rout.as<sfa::EvStreamOut>();
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        sess::Raw::Slot &x = r.slots[sl];
        if (x.fresh) memcpy(x.scaling, scaling + 3 * static_cast<size_t>(i), 3 * sizeof(double));
        x.fresh = 0;
        x.n += raw_off[i + 1] - raw_off[i];
        x.nev = ro[i].n_events;
        x.status = ro[i].status & 15;
        x.mean = ro[i].mean;
        x.sd = ro[i].sd;
        x.window = ro[i].window;
        if (au.on()) au.slots[sl] = sess::AutoStart::Slot{au.h_aout.as<sfa::EvAutoSlot>()[i], au.call[i].k_after, au.slots[sl].final_taken || au.call[i].final_now};
        // a recalibrated slot: its whole query was rewritten, so it is swept as a first chunk, which reads no carried row and
        // writes a new one (the planner never puts first and carried chunks into one wave).  A resweep session knows no other
        // sweep: q_new is the window then, and 0 in every call that leaves the window as it is
        if (ro[i].q_new > 0 && ro[i].q_first == 0) s->rows.len[sl] = 0;
        ch[i] = sfa::Chunk{static_cast<int64_t>(sl) * r.query + ro[i].q_first, ro[i].q_new};
    }
}

// the times of the stages in front of the sweep into the profile the sweep left, and the caller's info
int raw_fill_info(sfa_session *s, const int32_t *slot, int32_t n, sfa_session_raw_info_t *info) {
    sess::Raw &r = s->raw;
    float t_ev = 0, t_norm = 0;
    HIP_TRY(hipEventElapsedTime(&t_ev, r.ev_raw[0], r.ev_raw[1]));
    HIP_TRY(hipEventElapsedTime(&t_norm, r.ev_raw[1], r.ev_raw[2]));
    if (s->autos.on()) HIP_TRY(hipEventElapsedTime(&s->autos.ms, s->autos.ev_auto[0], s->autos.ev_auto[1]));
    s->c->prof.events_ms = t_ev;
    s->c->prof.normalise_ms = t_norm;
    s->c->prof.total_ms += t_ev + t_norm;
    const sfa::EvStreamOut *ro = r.h_rout.as<sfa::EvStreamOut>();
    for (int32_t i = 0; i < n; ++i) {
        const sess::Raw::Slot &x = r.slots[slot[i]];
        sfa_session_raw_info_t &f = info[i];
        f.n_samples = x.n;
        f.n_events = x.nev;
        f.q_events = s->rows.len[slot[i]];
        f.norm_mean = x.mean;
        f.norm_sd = x.sd;
        f.status = x.status | (ro[i].status & sfa::kRawResweep);
        f.norm_window = x.window;
    }
    return SFA_OK;
}

// ---- the two extend entry points in two halves: what a call is refused for, on the host alone, and the work.  A plain session
// runs one behind the other; a spread session asks every shard before any shard works, so a refused call changes no shard ----

int extend_check(sfa_session *s, const int32_t *slot, const float *events, const int64_t *ev_off, int32_t n) {
    if (s->resweep)
        return fail(SFA_EINVAL, "sfa_session_extend: the session was created with SFA_SESSION_RESWEEP: the caller's events are not kept, so nothing could be "
                                "swept again; it takes samples (sfa_session_raw_config, sfa_session_extend_raw)");
    if (s->raw.on) return fail(SFA_EINVAL, "sfa_session_extend: the session is in raw mode (sfa_session_raw_config): it takes samples, sfa_session_extend_raw");
    if (n == 0) return SFA_OK;
    begin_call(s);
    for (int32_t i = 0; i < n; ++i) {
        if (int rc = claim_slot(s, slot[i], "sfa_session_extend")) return rc;
        const int64_t l = ev_off[i + 1] - ev_off[i];
        if (l < 0) return fail(SFA_EINVAL, "sfa_session_extend: ev_off not monotone");
        if (s->rows.len[slot[i]] + l > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_extend: slot %d would hold more than 2^30 events", slot_name(s, slot[i]));
    }
    if (ev_off[n] - ev_off[0] > 0 && !events) return fail(SFA_EINVAL, "sfa_session_extend: null events");
    return SFA_OK;
}

int extend_run(sfa_session *s, const int32_t *slot, const float *events, const int64_t *ev_off, int32_t n, sfa_result_t *out) {
    sfa_ctx *c = s->c;
    const int64_t nq = ev_off[n] - ev_off[0];
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;  // a batch submitted and never waited for: its error words are this call's
    std::vector<sfa::Chunk> ch(n);
    for (int32_t i = 0; i < n; ++i) ch[i] = sfa::Chunk{ev_off[i] - ev_off[0], ev_off[i + 1] - ev_off[i]};
    return sweep_chunks(s, slot, ch.data(), n, events ? events + ev_off[0] : nullptr, nq, nullptr, out);
}

int extend_raw_check(sfa_session *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n) {
    if (!s->raw.on) return fail(SFA_EINVAL, "sfa_session_extend_raw: the session takes events (sfa_session_extend) until sfa_session_raw_config");
    return n == 0 ? static_cast<int>(SFA_OK) : raw_check(s, slot, raw, raw_off, scaling, n);
}

int extend_raw_run(sfa_session *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling, const uint8_t *end_of_read, int32_t n,
                   sfa_result_t *out, sfa_session_raw_info_t *info) {
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    if (int rc = raw_stage_tables(s, slot, raw_off, end_of_read, n)) return rc;
    if (int rc = raw_plan_points(s, slot, raw_off, end_of_read, n)) return rc;
    if (int rc = raw_launch_detector(s, raw, raw_off, n)) return rc;
    if (int rc = raw_launch_auto(s, n)) return rc;  // (retention and evaluation)
    if (int rc = raw_launch_norm(s, n)) return rc;
    std::vector<sfa::Chunk> ch(n);
    raw_take_results(s, slot, raw_off, scaling, n, ch.data());
    if (int rc = sweep_chunks(s, slot, ch.data(), n, nullptr, 0, s->raw.d_query.as<float>(), out)) return rc;
    return raw_fill_info(s, slot, n, info);
}

// ---- sfa_session_event_maps behind its argument checks: the rows idx[0..n_idx) of the caller's (nullptr: 0..n_idx-1), row
// idx[t] of slot slot_of[t]; its map goes to pairs + 2 * map_off[idx[t]] ----
int session_maps_rows(sfa_session *s, const sfa_result_t *rows, const int32_t *slot_of, const int32_t *idx, int32_t n_idx, const int64_t *map_off, int32_t *pairs,
                      int32_t *n_on_host) {
    static const char *const who = "sfa_session_event_maps";
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    if (s->keep.on())  // (the flags the keep kernel wrote; the wait below is the call's own)
        HIP_TRY(hipMemcpyAsync(s->keep.h_over.p, s->keep.d_over.p, static_cast<size_t>(s->n_slots), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    sess::Maps &mp = s->maps;
    if (int rc = mp.reserve(s->n_slots, static_cast<size_t>(n_idx))) return rc;
    // the query of a slot as swept: raw mode, its row of d_query (a resweep session stores the window in DP order already, so
    // nothing is reversed here); event mode, its kept events
    const int64_t stride = s->raw.on ? s->raw.query : s->keep.max_events;
    const float *base = s->raw.on ? s->raw.d_query.as<float>() : s->keep.d_keep.as<float>();
    for (int32_t sl = 0; sl < s->n_slots; ++sl) mp.q_off[sl] = sl * stride;
    for (int32_t t = 0; t < n_idx; ++t) {
        const int32_t k = idx ? idx[t] : t;
        mp.band[t].k = k;
        const sfa_result_t &r = rows[k];
        if (!r.valid || r.rid < 0) continue;  // no row (an empty or poisoned slot gives such rows): nothing is written
        const int32_t sl = slot_of[t];
        if (s->rows.poison[sl] || s->rows.len[sl] == 0)
            return fail(SFA_EINVAL, "%s: row %d: slot %d is empty or poisoned; it has no row in its current state", who, k, slot_name(s, sl));
        if (s->keep.on() && (s->keep.h_over.as<uint8_t>()[sl] || s->rows.len[sl] > s->keep.max_events))
            return fail(SFA_EINVAL, "%s: row %d: slot %d has received %lld events, more than the %d the session keeps; it has no maps until it is reset", who, k,
                        slot_name(s, sl), (long long)s->rows.len[sl], s->keep.max_events);
        if (int rc = sfa::map_row_band(c, r, k, s->rows.len[sl], map_off[k + 1] - map_off[k], who, "this reference", &mp.band[t])) return rc;
        mp.band[t].query = sl;
    }
    return sfa::event_maps_core(c, mp.scratch, base, mp.q_off.data(), mp.q_off.size(), false, mp.band.data(), n_idx, map_off, pairs, n_on_host);
}

// ---- spread sessions (SFA_SESSION_SPREAD on a group context): every entry point dealt to the shards' sub-sessions.  The rules
// are session_spread.hpp's, the visits (spread_deal, spread_run, spread_visit, spread_idle, spread_all) sfa_session_state.hpp's;
// here the prologue of each entry point: partition, the sub-calls side by side on the context's shard threads (for_each_shard:
// shard 0 on the caller's), the answers back in the caller's order.  Calls that touch no device (reset, lengths, the automatic
// start's records) visit the shards in turn on the caller's thread ----

int spread_create(sfa_ctx *g, int32_t n_slots, uint32_t flags, sfa_session **out) {
    if (n_slots <= 0) return fail(SFA_EINVAL, "sfa_session_create: n_slots must be positive, not %d", n_slots);
    if (flags & ~kSessionFlags) return fail(SFA_EINVAL, "sfa_session_create: unknown flag bits 0x%x", flags | SFA_SESSION_SPREAD);
    const int32_t G = static_cast<int32_t>(g->shards.size());
    std::unique_ptr<sfa_session> s(new sfa_session());
    s->c = g;
    s->n_slots = n_slots;
    s->track = !(flags & SFA_SESSION_NO_START);
    s->resweep = (flags & SFA_SESSION_RESWEEP) != 0;
    s->spread.reset(new sess::Spread());
    sess::Spread &sp = *s->spread;
    sp.subs.assign(static_cast<size_t>(G), nullptr);
    sp.shard.resize(static_cast<size_t>(G));
    for (int32_t r = 0; r < G; ++r) {
        const int32_t m = sfa::spread_slots_of(n_slots, r, G);
        if (m == 0) continue;  // (a session with fewer slots than shards: the trailing shards hold none)
        if (int rc = sfa_session_create(g->shards[r], m, flags, &sp.subs[r])) {  // this shard's code and message are the call's
            const std::string msg = sfa::last_error_slot();
            for (int32_t q = r - 1; q >= 0; --q) sfa_session_destroy(sp.subs[q]);
            sfa::last_error_slot() = msg;
            return rc;
        }
        sp.subs[r]->name_first = r;
        sp.subs[r]->name_step = G;
    }
    g->sessions.push_back(s.get());
    *out = s.release();
    return SFA_OK;
}

int spread_extend(sfa_session *s, const int32_t *slot, const float *events, const int64_t *ev_off, int32_t n, sfa_result_t *out) {
    static const char *const who = "sfa_session_extend";
    if (int rc = spread_live(s, who)) return rc;
    sess::Spread &sp = *s->spread;
    if (int rc = extend_check(sp.subs[0], nullptr, nullptr, nullptr, 0)) return rc;  // (the session's kind: the same on every shard)
    if (n == 0) return SFA_OK;
    if (int rc = spread_deal(s, slot, n, true, who)) return rc;
    sfa::spread_offsets(ev_off, &sp.part);
    if (int rc = spread_visit(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &) {
            return extend_check(sub, p.local.data(), events, p.off.data(), p.n());
        }))
        return rc;
    // events + absolute offsets cannot name a subset that is not contiguous: every shard's chunks are packed back to back
    return sfa::for_each_shard(s->c, [&](size_t r) {
        const sfa::SpreadShardPart &p = sp.part.shard[r];
        sess::Spread::Shard &b = sp.shard[r];
        if (p.n() == 0) return spread_idle(s->c->shards[r]);
        b.events.resize(static_cast<size_t>(std::max<int64_t>(p.off.back(), 1)));
        sfa::spread_pack(p, events, ev_off, b.events.data());
        b.rows.resize(p.local.size());
        if (int rc = extend_run(sp.subs[r], p.local.data(), b.events.data(), p.off.data(), p.n(), b.rows.data())) return rc;
        sfa::spread_scatter(p, b.rows.data(), out);
        return static_cast<int>(SFA_OK);
    });
}

int spread_extend_raw(sfa_session *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling, const uint8_t *end_of_read, int32_t n,
                      sfa_result_t *out, sfa_session_raw_info_t *info) {
    static const char *const who = "sfa_session_extend_raw";
    if (int rc = spread_live(s, who)) return rc;
    sess::Spread &sp = *s->spread;
    if (int rc = extend_raw_check(sp.subs[0], nullptr, nullptr, nullptr, nullptr, 0)) return rc;
    if (n == 0) return SFA_OK;
    if (int rc = spread_deal(s, slot, n, true, who)) return rc;
    sfa::spread_offsets(raw_off, &sp.part);
    if (int rc = spread_visit(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
            b.scaling.resize(3 * p.local.size());
            sfa::spread_gather(p, scaling, b.scaling.data(), 3);
            return extend_raw_check(sub, p.local.data(), raw, p.off.data(), b.scaling.data(), p.n());
        }))
        return rc;
    // (samples + absolute offsets: as for the events, a shard's chunks are packed back to back)
    return sfa::for_each_shard(s->c, [&](size_t r) {
        const sfa::SpreadShardPart &p = sp.part.shard[r];
        sess::Spread::Shard &b = sp.shard[r];
        if (p.n() == 0) return spread_idle(s->c->shards[r]);
        b.raw.resize(static_cast<size_t>(std::max<int64_t>(p.off.back(), 1)));
        sfa::spread_pack(p, raw, raw_off, b.raw.data());
        if (end_of_read) {
            b.end.resize(p.local.size());
            sfa::spread_gather(p, end_of_read, b.end.data());
        }
        b.rows.resize(p.local.size());
        b.info.resize(p.local.size());
        if (int rc = extend_raw_run(sp.subs[r], p.local.data(), b.raw.data(), p.off.data(), b.scaling.data(), end_of_read ? b.end.data() : nullptr, p.n(), b.rows.data(),
                                    b.info.data()))
            return rc;
        sfa::spread_scatter(p, b.rows.data(), out);
        sfa::spread_scatter(p, b.info.data(), info);
        return static_cast<int>(SFA_OK);
    });
}

int spread_reset(sfa_session *s, const int32_t *slot, int32_t n) {
    static const char *const who = "sfa_session_reset";
    if (int rc = spread_live(s, who)) return rc;
    if (!slot) {
        for (sfa_session *sub : s->spread->subs)
            if (sub) (void)sfa_session_reset(sub, nullptr, 0);
        return SFA_OK;
    }
    if (n < 0) return fail(SFA_EINVAL, "sfa_session_reset: negative count");
    if (int rc = spread_deal(s, slot, n, false, who)) return rc;
    return spread_visit(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &) { return sfa_session_reset(sub, p.local.data(), p.n()); });
}

int spread_lengths(sfa_session *s, const int32_t *slot, int32_t n, int64_t *len) {
    static const char *const who = "sfa_session_lengths";
    if (int rc = spread_live(s, who)) return rc;
    if (!slot && n != s->n_slots) return fail(SFA_EINVAL, "sfa_session_lengths: without a slot list n must be the session's %d slots, not %d", s->n_slots, n);
    if (int rc = spread_deal(s, slot, n, false, who)) return rc;  // (no list: every slot, in order)
    return spread_visit(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
        b.len.resize(p.local.size());
        if (int rc = sfa_session_lengths(sub, p.local.data(), p.n(), b.len.data())) return rc;
        sfa::spread_scatter(p, b.len.data(), len);
        return static_cast<int>(SFA_OK);
    });
}

int spread_candidates(sfa_session *s, const int32_t *slot, int32_t n, sfa_result_t *sec) {
    static const char *const who = "sfa_session_candidates";
    if (int rc = spread_live(s, who)) return rc;
    if (int rc = sfa_session_candidates(s->spread->subs[0], nullptr, 0, nullptr)) return rc;  // (a session that keeps none)
    if (int rc = spread_deal(s, slot, n, false, who)) return rc;
    return spread_run(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
        b.rows.resize(4 * p.local.size());
        if (int rc = sfa_session_candidates(sub, p.local.data(), p.n(), b.rows.data())) return rc;
        sfa::spread_scatter(p, b.rows.data(), sec, 4);
        return static_cast<int>(SFA_OK);
    });
}

int spread_query_span(sfa_session *s, const int32_t *slot, int32_t n, uint64_t *start_raw, uint64_t *end_raw) {
    static const char *const who = "sfa_session_query_span";
    if (int rc = spread_live(s, who)) return rc;
    if (int rc = sfa_session_query_span(s->spread->subs[0], nullptr, 0, nullptr, nullptr)) return rc;  // (a session that is not in raw mode)
    if (int rc = spread_deal(s, slot, n, false, who)) return rc;
    return spread_run(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
        const size_t m = p.local.size();
        b.span.resize(2 * m);
        if (int rc = sfa_session_query_span(sub, p.local.data(), p.n(), b.span.data(), b.span.data() + m)) return rc;
        sfa::spread_scatter(p, b.span.data(), start_raw);
        sfa::spread_scatter(p, b.span.data() + m, end_raw);
        return static_cast<int>(SFA_OK);
    });
}

int spread_auto_start(sfa_session *s, const int32_t *slot, int32_t n, sfa_session_auto_t *out) {
    static const char *const who = "sfa_session_auto_start";
    if (int rc = spread_live(s, who)) return rc;
    if (int rc = sfa_session_auto_start(s->spread->subs[0], nullptr, 0, nullptr)) return rc;  // (a session without the feature)
    if (int rc = spread_deal(s, slot, n, false, who)) return rc;
    return spread_visit(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
        b.autos.resize(p.local.size());
        if (int rc = sfa_session_auto_start(sub, p.local.data(), p.n(), b.autos.data())) return rc;
        sfa::spread_scatter(p, b.autos.data(), out);
        return static_cast<int>(SFA_OK);
    });
}

// the sub-session that owns *slot, which becomes its local number there (the one-slot calls: sfa_session_row, sfa_session_events)
int spread_owner(sfa_session *s, int32_t *slot, const char *who, sfa_session **sub) {
    if (int rc = spread_live(s, who)) return rc;
    if (*slot < 0 || *slot >= s->n_slots) return fail(SFA_EINVAL, "%s: slot %d out of range (the session has %d)", who, *slot, s->n_slots);
    const sfa::SpreadPlace at = sfa::spread_place(*slot, static_cast<int32_t>(s->c->shards.size()));
    *sub = s->spread->subs[at.shard];
    *slot = at.local;
    return SFA_OK;
}

// A configuration call that needs every slot empty: a slot in use is the one refusal that differs from shard to shard, so it is
// looked for on all of them before any shard hears of the call (spread_all)
template <typename F>
int spread_config(sfa_session *s, const char *who, F fn) {
    if (int rc = spread_live(s, who)) return rc;
    for (const sfa_session *sub : s->spread->subs)
        if (sub)
            if (const int32_t sl = first_busy_slot(sub); sl >= 0)
                return fail(SFA_EINVAL, "%s: slot %d is not empty; a session is configured only while every slot is (sfa_session_reset)", who, slot_name(sub, sl));
    return spread_all(s, who, fn);
}

int spread_event_maps(sfa_session *s, const sfa_result_t *rows, const int32_t *slot_of_row, int32_t n_rows, const int64_t *map_off, int32_t *pairs, int32_t *n_on_host) {
    static const char *const who = "sfa_session_event_maps";
    if (int rc = spread_live(s, who)) return rc;
    sess::Spread &sp = *s->spread;
    if (int rc = sfa_session_event_maps(sp.subs[0], nullptr, nullptr, 0, nullptr, nullptr, nullptr)) return rc;  // (a session that has no maps)
    if (int rc = spread_deal(s, slot_of_row, n_rows, false, who)) return rc;
    for (int32_t k = 0; k < n_rows; ++k)
        if (map_off[k + 1] < map_off[k] || map_off[k] < 0) return fail(SFA_EINVAL, "%s: map_off not monotone at row %d", who, k);
    // every shard writes its rows' pairs straight into the caller's, at the caller's map_off (as sfa_event_maps on a group context)
    const int rc = spread_run(s, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
        b.on_host = 0;
        return session_maps_rows(sub, rows, p.local.data(), p.index.data(), p.n(), map_off, pairs, &b.on_host);
    });
    if (!rc && n_on_host)
        for (size_t r = 0; r < sp.subs.size(); ++r)
            if (sp.part.shard[r].n() > 0) *n_on_host += sp.shard[r].on_host;
    return rc;
}

}  // namespace

namespace sfa {
void destroy_sessions(sfa_ctx *c) {
    while (!c->sessions.empty()) sfa_session_destroy(c->sessions.back());
}
}  // namespace sfa

extern "C" {

int64_t sfa_session_bytes(int64_t total_columns, int32_t n_slots, uint32_t session_flags) {
    if (total_columns <= 0 || n_slots <= 0 || (session_flags & ~kSessionFlags)) return SFA_EINVAL;
    // (SFA_SESSION_RESWEEP changes nothing here: a window beyond SFA_MAX_QUERY events runs as pieces over the carried row)
    const bool track = !(session_flags & SFA_SESSION_NO_START);
    if (total_columns > INT64_MAX / sess::Rows::slot_bytes(1, track) / n_slots) return SFA_ERANGE;
    return sess::Rows::slot_bytes(total_columns, track) * n_slots;
}

int sfa_session_create(sfa_ctx_t *c, int32_t n_slots, uint32_t session_flags, sfa_session_t **out) {
    if (!c || !out) return fail(SFA_EINVAL, "sfa_session_create: null argument");
    if (!c->shards.empty()) {
        if (!(session_flags & SFA_SESSION_SPREAD))
            return fail(SFA_EINVAL, "sfa_session_create: a session's rows live on one device; use a single-device context (sfa_init), or SFA_SESSION_SPREAD");
        return spread_create(c, n_slots, session_flags & ~static_cast<uint32_t>(SFA_SESSION_SPREAD), out);
    }
    // (on a single device SFA_SESSION_SPREAD changes nothing: the session is the plain one)
    if (c->flag & SFA_DTW) return fail(SFA_EINVAL, "sfa_session_create: sessions extend the subsequence DTW; the context has SFA_DTW");
    const bool resweep = (session_flags & SFA_SESSION_RESWEEP) != 0;  // (unknown bits beside it are refused below)
    if ((c->flag & SFA_RNA) && !(c->flag & SFA_INV) && !resweep)
        return fail(SFA_EINVAL, "sfa_session_create: with SFA_RNA and without SFA_INV the query rows are the events reversed, so new events "
                                "would become row 0; nothing carried over could be kept");
    if (n_slots <= 0) return fail(SFA_EINVAL, "sfa_session_create: n_slots must be positive, not %d", n_slots);
    if (session_flags & ~kSessionFlags) return fail(SFA_EINVAL, "sfa_session_create: unknown flag bits 0x%x", session_flags);
    if (sfa_session_bytes(c->model.total_cols, n_slots, session_flags) < 0) return fail(SFA_ENOMEM, "sfa_session_create: the carried rows do not fit");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<sfa_session> s(new sfa_session());
    s->c = c;
    s->n_slots = n_slots;
    s->track = !(session_flags & SFA_SESSION_NO_START);
    s->resweep = resweep;
    sess::Rows &r = s->rows;
    const size_t nj = c->model.n_jobs;
    if (int rc = r.reserve(c->model.total_cols, n_slots, nj, s->track)) return rc;
    if (int rc = s->sweep.reserve_count()) return rc;
    if (int rc = sess::create_events(s->sweep.ev, 4)) return rc;
    // every word the block loads of a sweep can see holds a cost (a large finite one), never a NaN (sdtw_session.hpp)
    HIP_TRY(hipMemsetAsync(r.d_row_c.p, 0x7f, r.d_row_c.cap, c->stream));
    if (s->track) HIP_TRY(hipMemsetAsync(r.d_row_s.p, 0, r.d_row_s.cap, c->stream));
    for (size_t j = 1; j < nj; ++j) r.h_col_off[j] = r.h_col_off[j - 1] + c->model.h_job_len[j - 1];  // ([0] is 0)
    HIP_TRY(hipMemcpyAsync(r.d_col_off.p, r.h_col_off.data(), 8 * nj, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sessions.push_back(s.get());
    *out = s.release();
    return SFA_OK;
}

int sfa_session_candidates_config(sfa_session_t *s, int32_t n_candidates) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_candidates_config: null session");
    if (n_candidates < 0 || n_candidates > 4) return fail(SFA_EINVAL, "sfa_session_candidates_config: n_candidates must be 0..4, not %d", n_candidates);
    if (s->spread) return spread_config(s, "sfa_session_candidates_config", [&](sfa_session *sub) { return sfa_session_candidates_config(sub, n_candidates); });
    if (const int32_t sl = first_busy_slot(s); sl >= 0)
        return fail(SFA_EINVAL, "sfa_session_candidates_config: slot %d is not empty; the lists are switched only while every slot is (sfa_session_reset)", slot_name(s, sl));
    if (n_candidates > 0) {
        sfa_ctx *c = s->c;
        HIP_TRY(hipSetDevice(c->device));
        if (int rc = s->cand.reserve(s->n_slots)) return rc;
        HIP_TRY(hipMemsetAsync(s->cand.d_cand.p, 0, sess::Candidates::bytes(s->n_slots), c->stream));  // (valid = 0; a slot's rows are written by its first sweep)
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    s->cand.n_cand = n_candidates;
    return SFA_OK;
}

int sfa_session_candidates(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_result_t *sec) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_candidates: null session");
    if (n < 0 || (n > 0 && (!slot || !sec))) return fail(SFA_EINVAL, "sfa_session_candidates: bad argument");
    if (s->spread) return spread_candidates(s, slot, n, sec);
    if (s->cand.n_cand == 0) return fail(SFA_EINVAL, "sfa_session_candidates: the session keeps no candidates (sfa_session_candidates_config)");
    if (int rc = check_slots(s, slot, n, "sfa_session_candidates")) return rc;
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(s->cand.h_cand.p, s->cand.d_cand.p, sess::Candidates::bytes(s->n_slots), hipMemcpyDeviceToHost, c->stream));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(SFA_EKERNEL, "sfa_session_candidates: the copy failed: %s", hipGetErrorString(hipGetLastError()));
    const sfa_result_t *cand = s->cand.h_cand.as<sfa_result_t>();
    for (int32_t i = 0; i < n; ++i) {  // (the reset is host-only: lengths and poison flags decide, as for the rows)
        const int32_t sl = slot[i];
        const bool none = s->rows.poison[sl] || s->rows.len[sl] == 0;
        for (int k = 0; k < 4; ++k) sec[4 * static_cast<size_t>(i) + k] = none ? kNoRow : cand[4 * static_cast<size_t>(sl) + k];
    }
    return SFA_OK;
}

int64_t sfa_session_row(sfa_session_t *s, int32_t slot, int32_t contig, int32_t strand_char, float *cost, int32_t *start) {
    if (!s || !cost) return fail(SFA_EINVAL, "sfa_session_row: null session or null cost");
    if (s->spread) {  // (the owning shard's)
        sfa_session *sub = nullptr;
        if (int rc = spread_owner(s, &slot, "sfa_session_row", &sub)) return rc;
        return sfa_session_row(sub, slot, contig, strand_char, cost, start);
    }
    sfa_ctx *c = s->c;
    if (int rc = check_slots(s, &slot, 1, "sfa_session_row")) return rc;
    if (contig < 0 || contig >= c->model.num_ref) return fail(SFA_EINVAL, "sfa_session_row: contig %d out of range (the reference has %d)", contig, c->model.num_ref);
    const int strands = c->model.n_jobs / c->model.num_ref;  // 1: RNA, forward arrays only
    if (strand_char != '+' && !(strand_char == '-' && strands == 2))
        return fail(SFA_EINVAL, "sfa_session_row: strand %d is neither '+' nor '-' (RNA has no '-')", strand_char);
    if (start && !s->track) return fail(SFA_EINVAL, "sfa_session_row: the session carries no start columns (SFA_SESSION_NO_START)");
    if (s->rows.poison[slot]) return fail(SFA_EINVAL, "sfa_session_row: slot %d is poisoned (a chunk held a NaN or inf); it has no row until it is reset", slot_name(s, slot));
    if (s->rows.len[slot] == 0) return fail(SFA_EINVAL, "sfa_session_row: slot %d has no events, so no carried row", slot_name(s, slot));
    const int32_t job = contig * strands + (strand_char == '-' ? 1 : 0);
    const int64_t n = c->model.h_job_len[job], row0 = sfa::kSessionPad + static_cast<int64_t>(slot) * c->model.total_cols + s->rows.h_col_off[job];
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(cost, s->rows.d_row_c.as<float>() + row0, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream));
    if (start) HIP_TRY(hipMemcpyAsync(start, s->rows.d_row_s.as<int32_t>() + row0, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return n;
}

void sfa_session_destroy(sfa_session_t *s) {
    if (!s) return;
    if (s->spread)  // (the sub-sessions first, each from its shard's list; then this one from the group's)
        for (sfa_session *sub : s->spread->subs) sfa_session_destroy(sub);
    sfa_ctx *c = s->c;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->sessions.erase(std::remove(c->sessions.begin(), c->sessions.end(), s), c->sessions.end());
    delete s;
}

int sfa_session_reset(sfa_session_t *s, const int32_t *slot, int32_t n) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_reset: null session");
    if (s->spread) return spread_reset(s, slot, n);
    if (!slot) {  // every slot
        for (int32_t sl = 0; sl < s->n_slots; ++sl) reset_slot(s, sl);
        return SFA_OK;
    }
    if (n < 0) return fail(SFA_EINVAL, "sfa_session_reset: negative count");
    if (int rc = check_slots(s, slot, n, "sfa_session_reset")) return rc;
    for (int32_t i = 0; i < n; ++i) reset_slot(s, slot[i]);
    return SFA_OK;
}

int sfa_session_lengths(sfa_session_t *s, const int32_t *slot, int32_t n, int64_t *len) {
    if (!s || !len || n < 0) return fail(SFA_EINVAL, "sfa_session_lengths: bad argument");
    if (s->spread) return spread_lengths(s, slot, n, len);
    if (!slot) {
        if (n != s->n_slots) return fail(SFA_EINVAL, "sfa_session_lengths: without a slot list n must be the session's %d slots, not %d", s->n_slots, n);
        std::copy(s->rows.len.begin(), s->rows.len.end(), len);
        return SFA_OK;
    }
    for (int32_t i = 0; i < n; ++i) {
        if (int rc = check_slots(s, slot + i, 1, "sfa_session_lengths")) return rc;
        len[i] = s->rows.len[slot[i]];
    }
    return SFA_OK;
}

int sfa_session_extend(sfa_session_t *s, const int32_t *slot, const float *events, const int64_t *ev_off, int32_t n, sfa_result_t *out) {
    if (!s || n < 0 || (n > 0 && (!slot || !ev_off || !out))) return fail(SFA_EINVAL, "sfa_session_extend: bad argument");
    if (s->spread) return spread_extend(s, slot, events, ev_off, n, out);
    if (int rc = extend_check(s, slot, events, ev_off, n)) return rc;
    return n == 0 ? static_cast<int>(SFA_OK) : extend_run(s, slot, events, ev_off, n, out);
}

// ---- event maps of a slot's row (the core: sfa_maps.hip) ----

int64_t sfa_session_keep_bytes(int32_t n_slots, int32_t max_events) {
    if (n_slots <= 0 || max_events <= 0) return SFA_EINVAL;
    const int64_t per_slot = sess::Keep::slot_bytes(max_events);
    if (per_slot > INT64_MAX / n_slots) return SFA_ERANGE;
    return per_slot * n_slots;
}

int sfa_session_keep_events(sfa_session_t *s, int32_t max_events) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_keep_events: null session");
    if (s->spread) return spread_config(s, "sfa_session_keep_events", [&](sfa_session *sub) { return sfa_session_keep_events(sub, max_events); });
    if (s->resweep || s->raw.on)
        return fail(SFA_EINVAL, "sfa_session_keep_events: a raw-mode session keeps its slots' queries already (sfa_session_raw_config); this is for event-mode sessions");
    if (max_events < 0 || max_events > INT32_MAX / 2) return fail(SFA_EINVAL, "sfa_session_keep_events: max_events must be 0 .. 2^30, not %d", max_events);
    if (const int32_t sl = first_busy_slot(s); sl >= 0)
        return fail(SFA_EINVAL, "sfa_session_keep_events: slot %d is not empty; events are kept from a slot's first chunk on, so it is switched only while every slot is empty (sfa_session_reset)", slot_name(s, sl));
    if (max_events > 0) {
        sfa_ctx *c = s->c;
        if (sfa_session_keep_bytes(s->n_slots, max_events) < 0) return fail(SFA_ENOMEM, "sfa_session_keep_events: the kept events do not fit");
        HIP_TRY(hipSetDevice(c->device));
        if (int rc = s->keep.reserve(s->n_slots, max_events)) return rc;
        HIP_TRY(hipMemsetAsync(s->keep.d_over.p, 0, static_cast<size_t>(s->n_slots), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    s->keep.max_events = max_events;
    return SFA_OK;
}

int sfa_session_event_maps(sfa_session_t *s, const sfa_result_t *rows, const int32_t *slot_of_row, int32_t n_rows, const int64_t *map_off, int32_t *pairs,
                           int32_t *n_on_host) {
    static const char *const who = "sfa_session_event_maps";
    if (!s || n_rows < 0 || (n_rows > 0 && (!rows || !slot_of_row || !map_off || !pairs))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (n_on_host) *n_on_host = 0;
    if (s->spread) return spread_event_maps(s, rows, slot_of_row, n_rows, map_off, pairs, n_on_host);
    if (!s->track) return fail(SFA_EINVAL, "%s: the session carries no start columns (SFA_SESSION_NO_START), so its rows have no band", who);
    if (!s->raw.on && !s->keep.on())
        return fail(SFA_EINVAL, "%s: an event-mode session does not keep the caller's events unless asked to (sfa_session_keep_events)", who);
    if (int rc = check_slots(s, slot_of_row, n_rows, who)) return rc;
    for (int32_t k = 0; k < n_rows; ++k)
        if (map_off[k + 1] < map_off[k] || map_off[k] < 0) return fail(SFA_EINVAL, "%s: map_off not monotone at row %d", who, k);
    if (n_rows == 0) return SFA_OK;
    return session_maps_rows(s, rows, slot_of_row, nullptr, n_rows, map_off, pairs, n_on_host);
}

// ---- raw mode: samples in, rows out (events_stream.hpp) ----

int64_t sfa_session_raw_bytes(int32_t n_slots, int32_t skip_events, int32_t query_events) {
    if (n_slots <= 0 || skip_events < 0 || query_events <= 0) return SFA_EINVAL;
    const int64_t per_slot = sess::Raw::slot_bytes(skip_events, query_events);
    if (per_slot > INT64_MAX / n_slots) return SFA_ERANGE;
    return per_slot * n_slots;
}

int sfa_session_raw_config(sfa_session_t *s, int32_t skip_events, int32_t norm_events, int32_t query_events) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_raw_config: null session");
    if (s->spread) return spread_config(s, "sfa_session_raw_config", [&](sfa_session *sub) { return sfa_session_raw_config(sub, skip_events, norm_events, query_events); });
    if (skip_events < 0 || norm_events < 25 || norm_events > query_events)
        return fail(SFA_EINVAL, "sfa_session_raw_config: need skip >= 0 and 25 <= norm <= query, not skip %d, norm %d, query %d", skip_events, norm_events, query_events);
    if (static_cast<int64_t>(skip_events) + query_events > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_raw_config: more than 2^30 events per slot");
    if (const int32_t sl = first_busy_slot(s); sl >= 0)
        return fail(SFA_EINVAL, "sfa_session_raw_config: slot %d is not empty; the mode of a session changes only while every slot is (sfa_session_reset)", slot_name(s, sl));
    HIP_TRY(hipSetDevice(s->c->device));
    if (sfa_session_raw_bytes(s->n_slots, skip_events, query_events) < 0) return fail(SFA_ENOMEM, "sfa_session_raw_config: the event tables do not fit");
    sess::Raw &r = s->raw;
    if (int rc = r.reserve(s->n_slots, skip_events, query_events)) return rc;
    if (int rc = sess::create_events(r.ev_raw, 3)) return rc;
    r.on = true;
    r.skip = skip_events;
    r.norm = norm_events;
    r.query = query_events;
    r.recal_n = 0;  // (the points were checked against the sizes that go)
    r.recal_flags = 0;
    s->autos.max_samples = s->autos.every = 0;  // (the automatic start was checked against the sizes that go)
    s->keep.max_events = 0;                     // (raw mode keeps the query itself)
    r.slots.assign(s->n_slots, sess::Raw::Slot{});
    return SFA_OK;
}

int64_t sfa_session_auto_bytes(int32_t n_slots, int32_t max_samples) {
    if (n_slots <= 0 || max_samples <= 0 || max_samples > sfa::kAutoMaxSamples) return SFA_EINVAL;
    const int64_t per_slot = sess::AutoStart::slot_bytes(max_samples);
    if (per_slot > INT64_MAX / n_slots) return SFA_ERANGE;
    return per_slot * n_slots;
}

int sfa_session_raw_auto_start(sfa_session_t *s, int32_t every_samples, int32_t max_samples, uint32_t flags) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: null session");
    if (s->spread) return spread_config(s, "sfa_session_raw_auto_start", [&](sfa_session *sub) { return sfa_session_raw_auto_start(sub, every_samples, max_samples, flags); });
    if (!s->raw.on) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: the session is not in raw mode (sfa_session_raw_config)");
    if (flags) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: unknown flag bits 0x%x", flags);
    if (every_samples < 0 || max_samples < 0 || max_samples > sfa::kAutoMaxSamples)
        return fail(SFA_EINVAL, "sfa_session_raw_auto_start: need every_samples >= 0 and 0 <= max_samples <= %d, not %d and %d", sfa::kAutoMaxSamples, every_samples,
                    max_samples);
    if (const int32_t sl = first_busy_slot(s); sl >= 0)
        return fail(SFA_EINVAL, "sfa_session_raw_auto_start: slot %d is not empty; the rule changes only while every slot is (sfa_session_reset)", slot_name(s, sl));
    sess::AutoStart &au = s->autos;
    if (max_samples == 0) {  // off
        au.max_samples = au.every = 0;
        return SFA_OK;
    }
    sfa_ctx *c = s->c;
    // the reference's own conditions of -p -1 (src/dtw_main.c:263-276), and the one kind of session that context can have
    if (!(c->flag & SFA_RNA)) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: DNA does not support auto query start detection (the context has no SFA_RNA)");
    if (c->flag & SFA_INV) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: inversion (SFA_INV) is not compatible with auto query start detection");
    if (c->flag & SFA_END) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: mapping from query end (SFA_END) is not compatible with auto query start detection");
    if (!s->resweep) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: the session was not created with SFA_SESSION_RESWEEP");
    if (s->raw.skip < sfa::kAutoFallback)
        return fail(SFA_EINVAL, "sfa_session_raw_auto_start: skip_events of sfa_session_raw_config is the largest skip a slot may resolve and must hold the fallback: need >= %d, not %d",
                    sfa::kAutoFallback, s->raw.skip);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = au.reserve(s->n_slots, max_samples)) return rc;
    if (int rc = sess::create_events(au.ev_auto, 2)) return rc;
    au.every = every_samples;
    au.max_samples = max_samples;
    au.ms = 0.0f;
    au.slots.assign(s->n_slots, sess::AutoStart::Slot{});
    au.call.resize(s->n_slots);
    return SFA_OK;
}

double sfa_session_auto_ms(sfa_session_t *s) {
    if (s && s->spread) {  // (the shards run side by side: the slowest)
        double ms = -1.0;
        for (sfa_session *sub : s->spread->subs) ms = std::max(ms, sfa_session_auto_ms(sub));
        return ms;
    }
    return (s && s->autos.on()) ? s->autos.ms : -1.0;
}

int sfa_session_auto_start(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_session_auto_t *out) {
    if (!s || n < 0 || (n > 0 && (!slot || !out))) return fail(SFA_EINVAL, "sfa_session_auto_start: bad argument");
    if (s->spread) return spread_auto_start(s, slot, n, out);
    if (!s->autos.on()) return fail(SFA_EINVAL, "sfa_session_auto_start: the session has no automatic query start (sfa_session_raw_auto_start)");
    for (int32_t i = 0; i < n; ++i) {
        if (int rc = check_slots(s, slot + i, 1, "sfa_session_auto_start")) return rc;
        const sfa::EvAutoSlot &a = s->autos.slots[slot[i]].h;
        out[i].target = a.target;
        out[i].frozen_at = a.frozen_at;
        out[i].skip = a.skip;
        out[i].status = a.status;
    }
    return SFA_OK;
}

int sfa_session_raw_recalibrate(sfa_session_t *s, const int32_t *at, int32_t n_at, uint32_t flags) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: null session");
    if (s->spread) return spread_config(s, "sfa_session_raw_recalibrate", [&](sfa_session *sub) { return sfa_session_raw_recalibrate(sub, at, n_at, flags); });
    if (!s->raw.on) return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: the session is not in raw mode (sfa_session_raw_config)");
    if (flags & ~static_cast<uint32_t>(SFA_RECAL_AT_END)) return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: unknown flag bits 0x%x", flags);
    if (const char *why = sfa::recal_list_error(at, n_at, s->raw.norm, s->raw.query))
        return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: %s; need norm < at[0] < ... < at[n - 1] <= query, at most %d points (norm %d, query %d)", why,
                    sfa::kRecalMaxPoints, s->raw.norm, s->raw.query);
    if (const int32_t sl = first_busy_slot(s); sl >= 0)
        return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: slot %d is not empty; the rule changes only while every slot is (sfa_session_reset)", slot_name(s, sl));
    static_assert(SFA_RECAL_AT_END == sfa::kRecalAtEnd, "the flag of the header is the rule's");
    for (int32_t k = 0; k < n_at; ++k) s->raw.recal_at[k] = at[k];
    s->raw.recal_n = n_at;
    s->raw.recal_flags = flags;
    return SFA_OK;
}

int64_t sfa_session_events(sfa_session_t *s, int32_t slot, int64_t first, sfa_event_t *out, int64_t cap) {
    if (s && s->spread) {  // (the owning shard's)
        sfa_session *sub = nullptr;
        if (int rc = spread_owner(s, &slot, "sfa_session_events", &sub)) return rc;
        return sfa_session_events(sub, slot, first, out, cap);
    }
    if (!s || !s->raw.on || first < 0 || cap < 0 || (cap > 0 && !out)) return fail(SFA_EINVAL, "sfa_session_events: bad argument (or the session is not in raw mode)");
    if (int rc = check_slots(s, &slot, 1, "sfa_session_events")) return rc;
    static_assert(sizeof(sfa_event_t) == sizeof(sfa::EvRecord), "the device table is copied out as it is");
    const int64_t nev = s->raw.slots[slot].nev, m = std::min<int64_t>(cap, nev - first);
    if (m > 0) {
        sfa_ctx *c = s->c;
        HIP_TRY(hipSetDevice(c->device));
        const sfa::EvRecord *src = s->raw.d_evtab.as<sfa::EvRecord>() + static_cast<int64_t>(slot) * s->raw.ev_cap() + first;
        HIP_TRY(hipMemcpyAsync(out, src, sizeof(sfa::EvRecord) * static_cast<size_t>(m), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return nev;
}

int sfa_session_query_span(sfa_session_t *s, const int32_t *slot, int32_t n, uint64_t *start_raw, uint64_t *end_raw) {
    if (!s || n < 0 || (n > 0 && (!slot || !start_raw || !end_raw))) return fail(SFA_EINVAL, "sfa_session_query_span: bad argument");
    if (s->spread) return spread_query_span(s, slot, n, start_raw, end_raw);
    if (!s->raw.on) return fail(SFA_EINVAL, "sfa_session_query_span: the session is not in raw mode (sfa_session_raw_config): it holds no event tables");
    if (int rc = check_slots(s, slot, n, "sfa_session_query_span")) return rc;
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    sess::Raw &r = s->raw;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nn = static_cast<size_t>(n);
    const bool per_slot = s->autos.on();
    const size_t in_bytes = (per_slot ? 12 : 8) * nn;  // (the third table, the slots' own skips, only with the automatic start)
    if (int rc = r.reserve_span(in_bytes, nn)) return rc;
    int32_t *h = r.h_span_in.as<int32_t>();
    for (int32_t i = 0; i < n; ++i) {  // (a slot reset since its last chunk has a stale table and no query)
        const int32_t sl = slot[i];
        h[i] = sl;
        h[nn + i] = (!r.slots[sl].fresh && (r.slots[sl].status & sfa::kRawCalibrated)) ? static_cast<int32_t>(s->rows.len[sl]) : 0;
        if (per_slot) h[2 * nn + i] = std::max(s->autos.slots[sl].h.skip, 0);  // (a calibrated slot has resolved its skip)
    }
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(r.d_span_in.p, h, in_bytes, hipMemcpyHostToDevice, st));
    sfa::EvSpanArgs a;
    a.slot = r.d_span_in.as<int32_t>();
    a.q_events = a.slot + nn;
    a.events = r.d_evtab.as<sfa::EvRecord>();
    a.span = r.d_span.as<uint64_t>();
    a.n = n;
    a.ev_cap = r.ev_cap();
    a.skip = r.skip;
    a.query_cap = r.query;
    a.skips = per_slot ? a.slot + 2 * nn : nullptr;
    if (per_slot)
        hipLaunchKernelGGL(sfa::ev_query_span_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL(sfa::ev_query_span_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, st, a);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(r.h_span.p, r.d_span.p, 16 * nn, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "sfa_session_query_span: the gather failed: %s", hipGetErrorString(hipGetLastError()));
    const uint64_t *sp = r.h_span.as<uint64_t>();
    for (int32_t i = 0; i < n; ++i) {
        start_raw[i] = sp[2 * i];
        end_raw[i] = sp[2 * i + 1];
    }
    return SFA_OK;
}

int sfa_session_extend_raw(sfa_session_t *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling,
                           const uint8_t *end_of_read, int32_t n, sfa_result_t *out, sfa_session_raw_info_t *info) {
    if (!s || n < 0 || (n > 0 && (!slot || !raw_off || !scaling || !out || !info))) return fail(SFA_EINVAL, "sfa_session_extend_raw: bad argument");
    if (s->spread) return spread_extend_raw(s, slot, raw, raw_off, scaling, end_of_read, n, out, info);
    if (int rc = extend_raw_check(s, slot, raw, raw_off, scaling, n)) return rc;
    return n == 0 ? static_cast<int>(SFA_OK) : extend_raw_run(s, slot, raw, raw_off, scaling, end_of_read, n, out, info);
}

}  // extern "C"
