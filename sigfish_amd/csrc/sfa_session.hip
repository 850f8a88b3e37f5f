// sfa_session.hip -- alignment sessions of the C-ABI (include/sigfish_amd.h): a slot's subsequence DTW extended chunk by chunk
// (sdtw_session.hpp).  The session owns the carried rows, the slots' lengths and poison flags, the current row of every slot and
// the staging of a call; it belongs to its context, runs on the context's stream and is freed with it at the latest.  In raw mode
// (sfa_session_raw_config) it also owns the slots' detector states, event tables and normalised queries (events_stream.hpp):
// samples go in, the events and the query stay on the device, and the sweep reads the new query events from there.
#include "sfa_ctx.hpp"
#define SFA_DEFINE_SESSION_KERNELS  // (this unit holds the plain kernel of sdtw_session.hpp)
#include "sdtw_session.hpp"
#include "events_stream.hpp"
#include "events_auto_stream.hpp"

namespace sfa {
// defined in sfa_align.hip, the unit that holds the plain kernels of sdtw_kernels.hpp
__global__ void sdtw_screen_kernel(const float *queries, const int64_t *q_off, const int n, uint8_t *bad, unsigned *count);
}  // namespace sfa

struct sfa_session {
    sfa_ctx *c = nullptr;
    int32_t n_slots = 0;
    bool track = true;  // start columns are carried (no SFA_SESSION_NO_START)
    bool resweep = false;  // SFA_SESSION_RESWEEP: raw mode only; a slot is swept when its window changes, over the window's events
    std::vector<int64_t> len;     // events every slot has received since its last reset
    std::vector<uint8_t> poison;  // a chunk of the slot held a NaN / inf: no rows until reset
    std::vector<int32_t> stamp;   // call in which the slot was named last (duplicates inside one call)
    int32_t call_no = 0;
    DevBuf d_row_c, d_row_s;      // carried rows: costs, start columns
    DevBuf d_col_off;             // [n_jobs] first column of every job inside a slot's row
    DevBuf d_rows;                // [n_slots] the slots' current rows
    PinBuf h_rows;
    DevBuf d_events, d_stage, d_bad, d_count, d_pbest, d_psecond, d_pend, d_pst;  // of a call
    PinBuf h_stage, h_bad;
    Event ev[4];  // first kernel, sweeps start / end, rows written
    int32_t n_cand = 0;           // sfa_session_candidates_config: candidates kept behind every slot's row (0: none, the plain kernels)
    DevBuf d_cand, d_p5;          // [n_slots][4] the slots' candidates; of a call: [n][n_jobs] lists of kTop5Words words
    PinBuf h_cand;
    // ---- raw mode ----
    bool raw = false;
    int32_t skip = 0, norm = 0, query = 0;
    std::vector<int64_t> raw_n;        // samples every slot has received since its last reset
    std::vector<int32_t> raw_nev;      // its final events
    std::vector<int32_t> raw_status;   // bits of sfa_session_raw_info_t.status
    std::vector<float> raw_mean, raw_sd;
    std::vector<int32_t> raw_window;   // events the slot's mean and sd span (0: not calibrated)
    std::vector<double> raw_scaling;   // [n_slots][3] latched by the first chunk after a reset
    std::vector<uint8_t> raw_fresh;    // no chunk since the last reset: the next one initialises the detector state
    DevBuf d_state, d_evtab, d_query;  // [n_slots] EvStreamSlot, [n_slots][skip + query] EvRecord, [n_slots][query] float
    DevBuf d_window;                   // [n_slots] i32: the window a calibrated slot's normalisation spans (EvNormArgs.window)
    int32_t recal_at[sfa::kRecalMaxPoints] = {0};  // sfa_session_raw_recalibrate: the points, their number, the flags
    int32_t recal_n = 0;
    uint32_t recal_flags = 0;
    DevBuf d_raw, d_rstage, d_rout;    // of a call: samples, entry tables, EvStreamOut per entry
    PinBuf h_rstage, h_rout;
    Event ev_raw[3];                   // detector start / end, normalisation end
    DevBuf d_span_in, d_span;          // of a sfa_session_query_span call: [slot n | q_events n (| skip n)] x i32, [n][2] u64
    PinBuf h_span_in, h_span;
    // ---- automatic query start (sfa_session_raw_auto_start); `skip` is then the largest skip a slot may resolve ----
    int32_t auto_every = 0, auto_max = 0;  // auto_max 0: off
    std::vector<sfa::EvAutoSlot> auto_h;   // what every slot's device state holds (read back by each call)
    std::vector<int32_t> auto_k;           // periodic points N_k a slot has passed
    std::vector<uint8_t> auto_final;       // its final point has been taken
    DevBuf d_auto, d_keep, d_csum, d_aout; // [n_slots] EvAutoSlot, [n_slots][auto_max] i16, of a call: prefix sums, EvAutoSlot per entry
    PinBuf h_aout;
    Event ev_auto[2];                      // retention + evaluation of a call: start, end
    double auto_ms = 0.0;                  // ... their time in the last call (sfa_session_auto_ms)
};

namespace {

int64_t row_words(int64_t total_columns, int32_t n_slots) { return total_columns * n_slots + 2 * sfa::kSessionPad; }

const sfa_result_t kNoRow = {-1, -1, -1, INFINITY, INFINITY, 0, 0, 0, 0};

// Where a slot's chunk lies in the device-resident event buffer of a call
struct Chunk {
    int64_t off, len;
};

// A piece of a slot's chunk inside one launch, and where the planner put it
struct Piece {
    int32_t call, slot, len, total, first, cls;
    int64_t off;
};

// One launch: the staging words of its tables, in the order of SessionArgs
struct Launch {
    std::vector<Piece> k;         // entries, in group order
    std::vector<int32_t> w_entry, g_qlen;
    sfa::SessionClass cls[sfa::kSessionMaxClasses];
    int32_t n_cls = 0, n_tasks = 0;
};

// groups of one launch: pieces sorted by (first chunk or not, class, length modulo R, length descending), 64 / lanes of them
// per wave as long as kind, class and length modulo R agree (MixedQuad's rule: every last row in the same lane and register)
void plan_launch(std::vector<Piece> &pieces, int32_t n_jobs, Launch *l) {
    for (Piece &p : pieces) p.cls = sfa::class_for(p.len);
    std::sort(pieces.begin(), pieces.end(), [](const Piece &a, const Piece &b) {
        if (a.first != b.first) return a.first > b.first;
        if (a.cls != b.cls) return a.cls < b.cls;
        const int R = sfa::kClassShapes[a.cls].R;
        if (a.len % R != b.len % R) return a.len % R < b.len % R;
        if (a.len != b.len) return a.len > b.len;
        return a.call < b.call;
    });
    l->k = pieces;
    l->n_cls = 0;
    int32_t n_groups = 0;
    for (size_t i = 0; i < pieces.size();) {
        const Piece &p = pieces[i];
        const sfa::ClassShape sh = sfa::kClassShapes[p.cls];
        if (l->n_cls == 0 || l->cls[l->n_cls - 1].first != p.first || l->cls[l->n_cls - 1].R != sh.R || l->cls[l->n_cls - 1].lanes != sh.lanes) {
            sfa::SessionClass &c = l->cls[l->n_cls++];
            c.R = sh.R;
            c.lanes = sh.lanes;
            c.first = p.first;
            c.group_base = n_groups;
            c.n_groups = 0;
            c.task_base = n_groups * n_jobs;
        }
        const int ns = 64 / sh.lanes;
        int32_t w[4] = {-1, -1, -1, -1};
        int m = 0;
        while (m < ns && i < pieces.size() && pieces[i].first == p.first && pieces[i].cls == p.cls && pieces[i].len % sh.R == p.len % sh.R) {
            w[m++] = static_cast<int32_t>(i++);
        }
        l->w_entry.insert(l->w_entry.end(), w, w + 4);
        l->g_qlen.push_back(p.len);  // (descending inside the run: the first is the longest)
        l->cls[l->n_cls - 1].n_groups++;
        ++n_groups;
    }
    l->n_tasks = n_groups * n_jobs;
}

size_t align8(size_t x) { return (x + 7) & ~static_cast<size_t>(7); }

constexpr uint32_t kSessionFlags = SFA_SESSION_NO_START | SFA_SESSION_RESWEEP;  // (0x2 is not assigned)

// raw mode: the slot's next chunk is marked fresh, and ev_stream_kernel then starts from the initial detector state
void reset_raw_slot(sfa_session *s, int32_t sl) {
    s->raw_n[sl] = 0;
    s->raw_nev[sl] = 0;
    s->raw_status[sl] = 0;
    s->raw_mean[sl] = s->raw_sd[sl] = 0.0f;
    s->raw_window[sl] = 0;
    s->raw_fresh[sl] = 1;
    if (s->auto_max > 0) {
        s->auto_h[sl] = sfa::EvAutoSlot{-1, -1, 0, sfa::kAutoPending};
        s->auto_k[sl] = 0;
        s->auto_final[sl] = 0;
    }
}

}  // namespace

namespace sfa {
void destroy_sessions(sfa_ctx *c) {
    while (!c->sessions.empty()) sfa_session_destroy(c->sessions.back());
}
}  // namespace sfa

// The core of both extend entry points: chunk i of the call, ch[i], is swept below the carried row of slot[i], and out[i] is the
// slot's row.  screen: the chunks are the nq host floats behind h_events (may be NULL when nq is 0), back to back; they are
// uploaded and screened for NaN / inf here.  Else they lie in d_events already (offsets of any kind), and d_bad holds the
// call's poison flags.
static int sweep_chunks(sfa_session *s, const int32_t *slot, const Chunk *ch, int32_t n, const float *h_events, int64_t nq, const float *d_events,
                        sfa_result_t *out) {
    sfa_ctx *c = s->c;
    const bool screen = d_events == nullptr;
    hipStream_t st = c->stream;
    const int32_t nj = c->model.n_jobs;

    // pieces: launch p holds events [p * 2048, (p + 1) * 2048) of every chunk that is that long
    std::vector<Launch> launches;
    std::vector<int32_t> call_slot(n, -1);
    int64_t new_events = 0;
    for (int32_t p = 0;; ++p) {
        std::vector<Piece> pieces;
        for (int32_t i = 0; i < n; ++i) {
            const int64_t l = ch[i].len, done = static_cast<int64_t>(p) * sfa::kMaxQuery;
            if (l <= done || s->poison[slot[i]]) continue;
            Piece k;
            k.call = i;
            k.slot = slot[i];
            k.len = static_cast<int32_t>(std::min<int64_t>(sfa::kMaxQuery, l - done));
            k.total = static_cast<int32_t>(s->len[slot[i]] + done + k.len);
            k.first = (s->len[slot[i]] + done == 0) ? 1 : 0;
            k.off = ch[i].off + done;
            k.cls = 0;
            pieces.push_back(k);
            if (p == 0) call_slot[i] = slot[i];
            new_events += k.len;
        }
        if (pieces.empty()) break;
        launches.emplace_back();
        plan_launch(pieces, nj, &launches.back());
    }

    // staging: [chunk offsets (n + 1) x i64 | call_slot n x i32 | per launch: k_off i64, w_entry, g_qlen, k_call, k_slot, k_len, k_total]
    size_t bytes = align8(8 * static_cast<size_t>(n + 1)) + align8(4 * static_cast<size_t>(n));
    for (const Launch &l : launches) bytes += 8 * l.k.size() + align8(4 * (l.w_entry.size() + l.g_qlen.size() + 4 * l.k.size()));
    const size_t n_part = static_cast<size_t>(n) * nj;
    // (d_bad: a raw call has reserved it for n entries and written it already; nothing is dropped here then)
    if (int rc = reserve_all(s->h_stage, bytes, s->d_stage, bytes, s->d_events, sizeof(float) * static_cast<size_t>(std::max<int64_t>(nq, 1)), s->d_bad,
                             static_cast<size_t>(n), s->h_bad, static_cast<size_t>(n) + 8, s->d_pbest, 4 * n_part, s->d_psecond, 4 * n_part, s->d_pend, 4 * n_part,
                             s->d_pst, 4 * n_part))
        return rc;
    if (s->n_cand > 0)
        if (int rc = s->d_p5.reserve(4 * sfa::kTop5Words * n_part)) return rc;
    char *h = s->h_stage.as<char>();
    const char *d = s->d_stage.as<char>();
    size_t at = 0;
    auto put = [&](const void *src, size_t nbytes) {
        const size_t here = at;
        if (nbytes) memcpy(h + at, src, nbytes);
        at += nbytes;
        return here;
    };
    std::vector<int64_t> rebased(n + 1);
    for (int32_t i = 0; i < n; ++i) rebased[i] = ch[i].off;  // (read by the screen only)
    rebased[n] = nq;
    const size_t o_evoff = put(rebased.data(), 8 * static_cast<size_t>(n + 1));
    at = align8(at);
    const size_t o_cslot = put(call_slot.data(), 4 * static_cast<size_t>(n));
    at = align8(at);
    std::vector<sfa::SessionArgs> args(launches.size());
    for (size_t li = 0; li < launches.size(); ++li) {
        const Launch &l = launches[li];
        const size_t m = l.k.size();
        std::vector<int64_t> k_off(m);
        std::vector<int32_t> k_call(m), k_slot(m), k_len(m), k_total(m);
        for (size_t i = 0; i < m; ++i) {
            k_off[i] = l.k[i].off;
            k_call[i] = l.k[i].call;
            k_slot[i] = l.k[i].slot;
            k_len[i] = l.k[i].len;
            k_total[i] = l.k[i].total;
        }
        sfa::SessionArgs &a = args[li];
        memset(&a, 0, sizeof a);
        a.k_off = reinterpret_cast<const int64_t *>(d + put(k_off.data(), 8 * m));
        a.w_entry = reinterpret_cast<const int32_t *>(d + put(l.w_entry.data(), 4 * l.w_entry.size()));
        a.g_qlen = reinterpret_cast<const int32_t *>(d + put(l.g_qlen.data(), 4 * l.g_qlen.size()));
        a.k_call = reinterpret_cast<const int32_t *>(d + put(k_call.data(), 4 * m));
        a.k_slot = reinterpret_cast<const int32_t *>(d + put(k_slot.data(), 4 * m));
        a.k_len = reinterpret_cast<const int32_t *>(d + put(k_len.data(), 4 * m));
        a.k_total = reinterpret_cast<const int32_t *>(d + put(k_total.data(), 4 * m));
        at = align8(at);
        a.events = screen ? s->d_events.as<float>() : d_events;
        a.bad = s->d_bad.as<uint8_t>();
        a.ref = c->model.d_ref.as<float>();
        a.job_off = c->model.d_job_off.as<int64_t>();
        a.job_len = c->model.d_job_len.as<int32_t>();
        a.col_off = s->d_col_off.as<int64_t>();
        a.row_c = s->d_row_c.as<float>();
        a.row_s = s->track ? s->d_row_s.as<int32_t>() : nullptr;
        a.row_stride = c->model.total_cols;
        a.p_best = s->d_pbest.as<float>();
        a.p_second = s->d_psecond.as<float>();
        a.p_end = s->d_pend.as<int32_t>();
        a.p_st = s->d_pst.as<int32_t>();
        for (int ci = 0; ci < l.n_cls; ++ci) a.cls[ci] = l.cls[ci];
        a.n_cls = l.n_cls;
        a.n_jobs = nj;
        a.n_tasks = l.n_tasks;
        a.p_top5 = s->n_cand > 0 ? s->d_p5.as<int32_t>() : nullptr;
    }
    if (at > bytes) return fail(SFA_EKERNEL, "session sweep: staging overrun (%zu > %zu)", at, bytes);
    HIP_TRY(hipMemcpyAsync(s->d_stage.p, h, at, hipMemcpyHostToDevice, st));
    if (screen && nq > 0) HIP_TRY(hipMemcpyAsync(s->d_events.p, h_events, sizeof(float) * nq, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->d_count.p, 0, 4, st));

    HIP_TRY(hipEventRecord(s->ev[0], st));
    // chunks with a NaN / inf event are not swept: the slot is poisoned (rows valid = 0 until reset)
    if (screen) {
        hipLaunchKernelGGL(sfa::sdtw_screen_kernel, dim3((n + 3) / 4), dim3(256), 0, st, s->d_events.as<float>(), reinterpret_cast<const int64_t *>(d + o_evoff), n,
                           s->d_bad.as<uint8_t>(), s->d_count.as<unsigned>());
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(s->ev[1], st));
    int64_t n_tasks = 0;
    for (const sfa::SessionArgs &a : args) {
        const dim3 grid((a.n_tasks + 3) / 4), block(256);
        if (s->n_cand > 0) {  // (every piece of a long chunk: the last one's list stays)
            if (s->track)
                hipLaunchKernelGGL((sfa::sdtw_session_kernel<true, true>), grid, block, 0, st, a);
            else
                hipLaunchKernelGGL((sfa::sdtw_session_kernel<false, true>), grid, block, 0, st, a);
        } else if (s->track)
            hipLaunchKernelGGL(sfa::sdtw_session_kernel<true>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(sfa::sdtw_session_kernel<false>, grid, block, 0, st, a);
        KERNEL_TRY();
        n_tasks += a.n_tasks;
    }
    HIP_TRY(hipEventRecord(s->ev[2], st));
    {
        sfa::SessionRowsArgs ra;
        ra.call_slot = reinterpret_cast<const int32_t *>(d + o_cslot);
        ra.bad = s->d_bad.as<uint8_t>();
        ra.p_best = s->d_pbest.as<float>();
        ra.p_second = s->d_psecond.as<float>();
        ra.p_end = s->d_pend.as<int32_t>();
        ra.p_st = s->d_pst.as<int32_t>();
        ra.job_contig = c->model.d_job_contig.as<int32_t>();
        ra.job_strand = c->model.d_job_strand.as<int8_t>();
        ra.ref_len = c->model.d_ref_len.as<int32_t>();
        ra.ref_st_offset = c->model.d_ref_off.as<int32_t>();
        ra.rows = s->d_rows.as<sfa::ResultRow>();
        ra.n_call = n;
        ra.n_jobs = nj;
        ra.track = s->track ? 1 : 0;
        hipLaunchKernelGGL(sfa::sdtw_session_rows_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ra);
        KERNEL_TRY();
        if (s->n_cand > 0 && !args.empty()) {  // (nothing swept: every slot keeps its candidates)
            sfa::SessionCandArgs ca;
            ca.call_slot = ra.call_slot;
            ca.bad = ra.bad;
            ca.p_top5 = s->d_p5.as<int32_t>();
            ca.job_contig = ra.job_contig;
            ca.job_strand = ra.job_strand;
            ca.ref_len = ra.ref_len;
            ca.ref_st_offset = ra.ref_st_offset;
            ca.cand = s->d_cand.as<sfa::ResultRow>();
            ca.n_call = n;
            ca.n_jobs = nj;
            ca.n_cand = s->n_cand;
            ca.track = ra.track;
            hipLaunchKernelGGL(sfa::sdtw_session_cand_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ca);
            KERNEL_TRY();
        }
    }
    HIP_TRY(hipEventRecord(s->ev[3], st));
    HIP_TRY(hipMemcpyAsync(s->h_rows.p, s->d_rows.p, sizeof(sfa_result_t) * s->n_slots, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s->h_bad.p, s->d_bad.p, static_cast<size_t>(n), hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "session sweep: the launches failed: %s", hipGetErrorString(hipGetLastError()));

    const uint8_t *bad = s->h_bad.as<uint8_t>();
    const sfa_result_t *rows = s->h_rows.as<sfa_result_t>();
    int64_t non_finite = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        s->len[sl] += ch[i].len;
        if (bad[i]) s->poison[sl] = 1;
        non_finite += s->poison[sl];
        out[i] = (s->poison[sl] || s->len[sl] == 0) ? kNoRow : rows[sl];
    }
    float t_fill = 0, t_total = 0;
    HIP_TRY(hipEventElapsedTime(&t_fill, s->ev[1], s->ev[2]));
    HIP_TRY(hipEventElapsedTime(&t_total, s->ev[0], s->ev[3]));
    sfa_profile_t pr{};
    pr.fill_ms = t_fill;
    pr.total_ms = t_total;
    pr.finalize_ms = t_total - t_fill;
    pr.cells = new_events * c->model.total_cols;
    pr.fill_launches = static_cast<int64_t>(args.size());
    pr.n_tasks = n_tasks;
    pr.n_chunks = nj;
    pr.n_segments = 1;
    pr.non_finite_reads = non_finite;
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    c->prof = pr;
    return SFA_OK;
}

extern "C" {

int64_t sfa_session_bytes(int64_t total_columns, int32_t n_slots, uint32_t session_flags) {
    if (total_columns <= 0 || n_slots <= 0 || (session_flags & ~kSessionFlags)) return SFA_EINVAL;
    // (SFA_SESSION_RESWEEP changes nothing here: a window beyond SFA_MAX_QUERY events runs as pieces over the carried row)
    const int64_t per_column = (session_flags & SFA_SESSION_NO_START) ? 4 : 8;
    if (total_columns > INT64_MAX / per_column / n_slots) return SFA_ERANGE;
    return total_columns * n_slots * per_column;  // one row per slot, updated in place
}

int sfa_session_create(sfa_ctx_t *c, int32_t n_slots, uint32_t session_flags, sfa_session_t **out) {
    if (!c || !out) return fail(SFA_EINVAL, "sfa_session_create: null argument");
    if (!c->shards.empty()) return fail(SFA_EINVAL, "sfa_session_create: a session's rows live on one device; use a single-device context (sfa_init)");
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
    s->len.assign(n_slots, 0);
    s->poison.assign(n_slots, 0);
    s->stamp.assign(n_slots, 0);
    const size_t words = static_cast<size_t>(row_words(c->model.total_cols, n_slots));
    const size_t nj = c->model.n_jobs;
    if (int rc = reserve_all(s->d_row_c, 4 * words, s->d_col_off, 8 * nj, s->d_rows, sizeof(sfa_result_t) * n_slots, s->h_rows,
                             sizeof(sfa_result_t) * n_slots, s->d_count, 64))
        return rc;
    if (s->track)
        if (int rc = s->d_row_s.reserve(4 * words)) return rc;
    for (Event &e : s->ev)
        if (hipEventCreate(&e.h) != hipSuccess) return fail(SFA_ENODEV, "hipEventCreate failed");
    // every word the block loads of a sweep can see holds a cost (a large finite one), never a NaN (sdtw_session.hpp)
    HIP_TRY(hipMemsetAsync(s->d_row_c.p, 0x7f, s->d_row_c.cap, c->stream));
    if (s->track) HIP_TRY(hipMemsetAsync(s->d_row_s.p, 0, s->d_row_s.cap, c->stream));
    std::vector<int64_t> col_off(nj);
    int64_t acc = 0;
    for (size_t j = 0; j < nj; ++j) {
        col_off[j] = acc;
        acc += c->model.h_job_len[j];
    }
    HIP_TRY(hipMemcpyAsync(s->d_col_off.p, col_off.data(), 8 * nj, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (col_off leaves scope)
    c->sessions.push_back(s.get());
    *out = s.release();
    return SFA_OK;
}

int sfa_session_candidates_config(sfa_session_t *s, int32_t n_candidates) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_candidates_config: null session");
    if (n_candidates < 0 || n_candidates > 4) return fail(SFA_EINVAL, "sfa_session_candidates_config: n_candidates must be 0..4, not %d", n_candidates);
    for (int32_t sl = 0; sl < s->n_slots; ++sl)
        if (s->len[sl] != 0 || s->poison[sl] || (s->raw && !s->raw_fresh[sl]))
            return fail(SFA_EINVAL, "sfa_session_candidates_config: slot %d is not empty; the lists are switched only while every slot is (sfa_session_reset)", sl);
    if (n_candidates > 0) {
        sfa_ctx *c = s->c;
        HIP_TRY(hipSetDevice(c->device));
        const size_t bytes = sizeof(sfa_result_t) * 4 * static_cast<size_t>(s->n_slots);
        if (int rc = reserve_all(s->d_cand, bytes, s->h_cand, bytes)) return rc;
        HIP_TRY(hipMemsetAsync(s->d_cand.p, 0, bytes, c->stream));  // (valid = 0; a slot's rows are written by its first sweep)
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    s->n_cand = n_candidates;
    return SFA_OK;
}

int sfa_session_candidates(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_result_t *sec) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_candidates: null session");
    if (n < 0 || (n > 0 && (!slot || !sec))) return fail(SFA_EINVAL, "sfa_session_candidates: bad argument");
    if (s->n_cand == 0) return fail(SFA_EINVAL, "sfa_session_candidates: the session keeps no candidates (sfa_session_candidates_config)");
    for (int32_t i = 0; i < n; ++i)
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_candidates: slot %d out of range (the session has %d)", slot[i], s->n_slots);
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(s->h_cand.p, s->d_cand.p, sizeof(sfa_result_t) * 4 * static_cast<size_t>(s->n_slots), hipMemcpyDeviceToHost, c->stream));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(SFA_EKERNEL, "sfa_session_candidates: the copy failed: %s", hipGetErrorString(hipGetLastError()));
    const sfa_result_t *cand = s->h_cand.as<sfa_result_t>();
    for (int32_t i = 0; i < n; ++i) {  // (the reset is host-only: lengths and poison flags decide, as for the rows)
        const int32_t sl = slot[i];
        const bool none = s->poison[sl] || s->len[sl] == 0;
        for (int k = 0; k < 4; ++k) sec[4 * static_cast<size_t>(i) + k] = none ? kNoRow : cand[4 * static_cast<size_t>(sl) + k];
    }
    return SFA_OK;
}

int64_t sfa_session_row(sfa_session_t *s, int32_t slot, int32_t contig, int32_t strand_char, float *cost, int32_t *start) {
    if (!s || !cost) return fail(SFA_EINVAL, "sfa_session_row: null session or null cost");
    sfa_ctx *c = s->c;
    if (slot < 0 || slot >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_row: slot %d out of range (the session has %d)", slot, s->n_slots);
    if (contig < 0 || contig >= c->model.num_ref) return fail(SFA_EINVAL, "sfa_session_row: contig %d out of range (the reference has %d)", contig, c->model.num_ref);
    const int strands = c->model.n_jobs / c->model.num_ref;  // 1: RNA, forward arrays only
    if (strand_char != '+' && !(strand_char == '-' && strands == 2))
        return fail(SFA_EINVAL, "sfa_session_row: strand %d is neither '+' nor '-' (RNA has no '-')", strand_char);
    if (start && !s->track) return fail(SFA_EINVAL, "sfa_session_row: the session carries no start columns (SFA_SESSION_NO_START)");
    if (s->poison[slot]) return fail(SFA_EINVAL, "sfa_session_row: slot %d is poisoned (a chunk held a NaN or inf); it has no row until it is reset", slot);
    if (s->len[slot] == 0) return fail(SFA_EINVAL, "sfa_session_row: slot %d has no events, so no carried row", slot);
    const int32_t job = contig * strands + (strand_char == '-' ? 1 : 0);
    int64_t col_off = 0;
    for (int32_t j = 0; j < job; ++j) col_off += c->model.h_job_len[j];
    const int64_t n = c->model.h_job_len[job], row0 = sfa::kSessionPad + static_cast<int64_t>(slot) * c->model.total_cols + col_off;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(cost, s->d_row_c.as<float>() + row0, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream));
    if (start) HIP_TRY(hipMemcpyAsync(start, s->d_row_s.as<int32_t>() + row0, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return n;
}

void sfa_session_destroy(sfa_session_t *s) {
    if (!s) return;
    sfa_ctx *c = s->c;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->sessions.erase(std::remove(c->sessions.begin(), c->sessions.end(), s), c->sessions.end());
    delete s;
}

int sfa_session_reset(sfa_session_t *s, const int32_t *slot, int32_t n) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_reset: null session");
    if (!slot) {  // every slot
        std::fill(s->len.begin(), s->len.end(), 0);
        std::fill(s->poison.begin(), s->poison.end(), 0);
        if (s->raw)
            for (int32_t sl = 0; sl < s->n_slots; ++sl) reset_raw_slot(s, sl);
        return SFA_OK;
    }
    if (n < 0) return fail(SFA_EINVAL, "sfa_session_reset: negative count");
    for (int32_t i = 0; i < n; ++i)
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_reset: slot %d out of range (the session has %d)", slot[i], s->n_slots);
    for (int32_t i = 0; i < n; ++i) {  // (a slot's next chunk is a first chunk: nothing of its carried row is read)
        s->len[slot[i]] = 0;
        s->poison[slot[i]] = 0;
        if (s->raw) reset_raw_slot(s, slot[i]);
    }
    return SFA_OK;
}

int sfa_session_lengths(sfa_session_t *s, const int32_t *slot, int32_t n, int64_t *len) {
    if (!s || !len || n < 0) return fail(SFA_EINVAL, "sfa_session_lengths: bad argument");
    if (!slot) {
        if (n != s->n_slots) return fail(SFA_EINVAL, "sfa_session_lengths: without a slot list n must be the session's %d slots, not %d", s->n_slots, n);
        std::copy(s->len.begin(), s->len.end(), len);
        return SFA_OK;
    }
    for (int32_t i = 0; i < n; ++i) {
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_lengths: slot %d out of range (the session has %d)", slot[i], s->n_slots);
        len[i] = s->len[slot[i]];
    }
    return SFA_OK;
}

int sfa_session_extend(sfa_session_t *s, const int32_t *slot, const float *events, const int64_t *ev_off, int32_t n, sfa_result_t *out) {
    if (!s || n < 0 || (n > 0 && (!slot || !ev_off || !out))) return fail(SFA_EINVAL, "sfa_session_extend: bad argument");
    if (s->resweep)
        return fail(SFA_EINVAL, "sfa_session_extend: the session was created with SFA_SESSION_RESWEEP: the caller's events are not kept, so nothing could be "
                                "swept again; it takes samples (sfa_session_raw_config, sfa_session_extend_raw)");
    if (s->raw) return fail(SFA_EINVAL, "sfa_session_extend: the session is in raw mode (sfa_session_raw_config): it takes samples, sfa_session_extend_raw");
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    if (++s->call_no == INT32_MAX) {
        std::fill(s->stamp.begin(), s->stamp.end(), 0);
        s->call_no = 1;
    }
    for (int32_t i = 0; i < n; ++i) {
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_extend: slot %d out of range (the session has %d)", slot[i], s->n_slots);
        if (s->stamp[slot[i]] == s->call_no) return fail(SFA_EINVAL, "sfa_session_extend: slot %d is named twice in one call", slot[i]);
        s->stamp[slot[i]] = s->call_no;
        const int64_t l = ev_off[i + 1] - ev_off[i];
        if (l < 0) return fail(SFA_EINVAL, "sfa_session_extend: ev_off not monotone");
        if (s->len[slot[i]] + l > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_extend: slot %d would hold more than 2^30 events", slot[i]);
    }
    const int64_t nq = ev_off[n] - ev_off[0];
    if (nq > 0 && !events) return fail(SFA_EINVAL, "sfa_session_extend: null events");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;  // a batch submitted and never waited for: its error words are this call's
    std::vector<Chunk> ch(n);
    for (int32_t i = 0; i < n; ++i) ch[i] = Chunk{ev_off[i] - ev_off[0], ev_off[i + 1] - ev_off[i]};
    return sweep_chunks(s, slot, ch.data(), n, events ? events + ev_off[0] : nullptr, nq, nullptr, out);
}

// ---- raw mode: samples in, rows out (events_stream.hpp) ----

int64_t sfa_session_raw_bytes(int32_t n_slots, int32_t skip_events, int32_t query_events) {
    if (n_slots <= 0 || skip_events < 0 || query_events <= 0) return SFA_EINVAL;
    const int64_t cap = static_cast<int64_t>(skip_events) + query_events;
    const int64_t per_slot = cap * static_cast<int64_t>(sizeof(sfa::EvRecord)) + 4 * static_cast<int64_t>(query_events) + static_cast<int64_t>(sizeof(sfa::EvStreamSlot));
    if (per_slot > INT64_MAX / n_slots) return SFA_ERANGE;
    return per_slot * n_slots;
}

int sfa_session_raw_config(sfa_session_t *s, int32_t skip_events, int32_t norm_events, int32_t query_events) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_raw_config: null session");
    if (skip_events < 0 || norm_events < 25 || norm_events > query_events)
        return fail(SFA_EINVAL, "sfa_session_raw_config: need skip >= 0 and 25 <= norm <= query, not skip %d, norm %d, query %d", skip_events, norm_events, query_events);
    if (static_cast<int64_t>(skip_events) + query_events > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_raw_config: more than 2^30 events per slot");
    for (int32_t sl = 0; sl < s->n_slots; ++sl)
        if (s->len[sl] != 0 || s->poison[sl] || (s->raw && !s->raw_fresh[sl]))
            return fail(SFA_EINVAL, "sfa_session_raw_config: slot %d is not empty; the mode of a session changes only while every slot is (sfa_session_reset)", sl);
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    const size_t ns = static_cast<size_t>(s->n_slots), cap = static_cast<size_t>(skip_events) + query_events;
    if (sfa_session_raw_bytes(s->n_slots, skip_events, query_events) < 0) return fail(SFA_ENOMEM, "sfa_session_raw_config: the event tables do not fit");
    if (int rc = reserve_all(s->d_state, sizeof(sfa::EvStreamSlot) * ns, s->d_evtab, sizeof(sfa::EvRecord) * cap * ns, s->d_query, 4 * static_cast<size_t>(query_events) * ns,
                             s->d_window, 4 * ns))
        return rc;
    for (Event &e : s->ev_raw)
        if (!e.h && hipEventCreate(&e.h) != hipSuccess) return fail(SFA_ENODEV, "hipEventCreate failed");
    s->raw = true;
    s->skip = skip_events;
    s->norm = norm_events;
    s->query = query_events;
    s->raw_n.assign(ns, 0);
    s->raw_nev.assign(ns, 0);
    s->raw_status.assign(ns, 0);
    s->raw_mean.assign(ns, 0.0f);
    s->raw_sd.assign(ns, 0.0f);
    s->raw_window.assign(ns, 0);
    s->recal_n = 0;  // (the points were checked against the sizes that go)
    s->recal_flags = 0;
    s->raw_scaling.assign(3 * ns, 0.0);
    s->raw_fresh.assign(ns, 1);
    s->auto_max = s->auto_every = 0;  // (the automatic start was checked against the sizes that go)
    return SFA_OK;
}

int64_t sfa_session_auto_bytes(int32_t n_slots, int32_t max_samples) {
    if (n_slots <= 0 || max_samples <= 0 || max_samples > sfa::kAutoMaxSamples) return SFA_EINVAL;
    // retention (int16), the slot's state, and the prefix sums of a call in which every slot has a pending point
    const int64_t per_slot = 2 * static_cast<int64_t>(max_samples) + static_cast<int64_t>(sizeof(sfa::EvAutoSlot)) + 4 * (static_cast<int64_t>(max_samples) + 1);
    if (per_slot > INT64_MAX / n_slots) return SFA_ERANGE;
    return per_slot * n_slots;
}

int sfa_session_raw_auto_start(sfa_session_t *s, int32_t every_samples, int32_t max_samples, uint32_t flags) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: null session");
    if (!s->raw) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: the session is not in raw mode (sfa_session_raw_config)");
    if (flags) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: unknown flag bits 0x%x", flags);
    if (every_samples < 0 || max_samples < 0 || max_samples > sfa::kAutoMaxSamples)
        return fail(SFA_EINVAL, "sfa_session_raw_auto_start: need every_samples >= 0 and 0 <= max_samples <= %d, not %d and %d", sfa::kAutoMaxSamples, every_samples,
                    max_samples);
    for (int32_t sl = 0; sl < s->n_slots; ++sl)
        if (s->len[sl] != 0 || s->poison[sl] || !s->raw_fresh[sl])
            return fail(SFA_EINVAL, "sfa_session_raw_auto_start: slot %d is not empty; the rule changes only while every slot is (sfa_session_reset)", sl);
    if (max_samples == 0) {  // off
        s->auto_max = s->auto_every = 0;
        return SFA_OK;
    }
    sfa_ctx *c = s->c;
    // the reference's own conditions of -p -1 (src/dtw_main.c:263-276), and the one kind of session that context can have
    if (!(c->flag & SFA_RNA)) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: DNA does not support auto query start detection (the context has no SFA_RNA)");
    if (c->flag & SFA_INV) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: inversion (SFA_INV) is not compatible with auto query start detection");
    if (c->flag & SFA_END) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: mapping from query end (SFA_END) is not compatible with auto query start detection");
    if (!s->resweep) return fail(SFA_EINVAL, "sfa_session_raw_auto_start: the session was not created with SFA_SESSION_RESWEEP");
    if (s->skip < sfa::kAutoFallback)
        return fail(SFA_EINVAL, "sfa_session_raw_auto_start: skip_events of sfa_session_raw_config is the largest skip a slot may resolve and must hold the fallback: need >= %d, not %d",
                    sfa::kAutoFallback, s->skip);
    HIP_TRY(hipSetDevice(c->device));
    const size_t ns = static_cast<size_t>(s->n_slots);
    if (int rc = reserve_all(s->d_auto, sizeof(sfa::EvAutoSlot) * ns, s->d_keep, 2 * static_cast<size_t>(max_samples) * ns)) return rc;
    for (Event &e : s->ev_auto)
        if (!e.h && hipEventCreate(&e.h) != hipSuccess) return fail(SFA_ENODEV, "hipEventCreate failed");
    s->auto_every = every_samples;
    s->auto_max = max_samples;
    s->auto_ms = 0.0;
    s->auto_h.assign(ns, sfa::EvAutoSlot{-1, -1, 0, sfa::kAutoPending});
    s->auto_k.assign(ns, 0);
    s->auto_final.assign(ns, 0);
    return SFA_OK;
}

double sfa_session_auto_ms(sfa_session_t *s) { return (s && s->auto_max > 0) ? s->auto_ms : -1.0; }

int sfa_session_auto_start(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_session_auto_t *out) {
    if (!s || n < 0 || (n > 0 && (!slot || !out))) return fail(SFA_EINVAL, "sfa_session_auto_start: bad argument");
    if (s->auto_max == 0) return fail(SFA_EINVAL, "sfa_session_auto_start: the session has no automatic query start (sfa_session_raw_auto_start)");
    for (int32_t i = 0; i < n; ++i) {
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_auto_start: slot %d out of range (the session has %d)", slot[i], s->n_slots);
        const sfa::EvAutoSlot &a = s->auto_h[slot[i]];
        out[i].target = a.target;
        out[i].frozen_at = a.frozen_at;
        out[i].skip = a.skip;
        out[i].status = a.status;
    }
    return SFA_OK;
}

int sfa_session_raw_recalibrate(sfa_session_t *s, const int32_t *at, int32_t n_at, uint32_t flags) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: null session");
    if (!s->raw) return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: the session is not in raw mode (sfa_session_raw_config)");
    if (flags & ~static_cast<uint32_t>(SFA_RECAL_AT_END)) return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: unknown flag bits 0x%x", flags);
    if (const char *why = sfa::recal_list_error(at, n_at, s->norm, s->query))
        return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: %s; need norm < at[0] < ... < at[n - 1] <= query, at most %d points (norm %d, query %d)", why,
                    sfa::kRecalMaxPoints, s->norm, s->query);
    for (int32_t sl = 0; sl < s->n_slots; ++sl)
        if (s->len[sl] != 0 || s->poison[sl] || !s->raw_fresh[sl])
            return fail(SFA_EINVAL, "sfa_session_raw_recalibrate: slot %d is not empty; the rule changes only while every slot is (sfa_session_reset)", sl);
    static_assert(SFA_RECAL_AT_END == sfa::kRecalAtEnd, "the flag of the header is the rule's");
    for (int32_t k = 0; k < n_at; ++k) s->recal_at[k] = at[k];
    s->recal_n = n_at;
    s->recal_flags = flags;
    return SFA_OK;
}

int64_t sfa_session_events(sfa_session_t *s, int32_t slot, int64_t first, sfa_event_t *out, int64_t cap) {
    if (!s || !s->raw || first < 0 || cap < 0 || (cap > 0 && !out)) return fail(SFA_EINVAL, "sfa_session_events: bad argument (or the session is not in raw mode)");
    if (slot < 0 || slot >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_events: slot %d out of range (the session has %d)", slot, s->n_slots);
    static_assert(sizeof(sfa_event_t) == sizeof(sfa::EvRecord), "the device table is copied out as it is");
    const int64_t nev = s->raw_nev[slot], m = std::min<int64_t>(cap, nev - first);
    if (m > 0) {
        sfa_ctx *c = s->c;
        HIP_TRY(hipSetDevice(c->device));
        const sfa::EvRecord *src = s->d_evtab.as<sfa::EvRecord>() + static_cast<int64_t>(slot) * (s->skip + s->query) + first;
        HIP_TRY(hipMemcpyAsync(out, src, sizeof(sfa::EvRecord) * static_cast<size_t>(m), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return nev;
}

int sfa_session_query_span(sfa_session_t *s, const int32_t *slot, int32_t n, uint64_t *start_raw, uint64_t *end_raw) {
    if (!s || n < 0 || (n > 0 && (!slot || !start_raw || !end_raw))) return fail(SFA_EINVAL, "sfa_session_query_span: bad argument");
    if (!s->raw) return fail(SFA_EINVAL, "sfa_session_query_span: the session is not in raw mode (sfa_session_raw_config): it holds no event tables");
    for (int32_t i = 0; i < n; ++i)
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_query_span: slot %d out of range (the session has %d)", slot[i], s->n_slots);
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nn = static_cast<size_t>(n);
    const bool per_slot = s->auto_max > 0;
    const size_t in_bytes = (per_slot ? 12 : 8) * nn;  // (the third table, the slots' own skips, only with the automatic start)
    if (int rc = reserve_all(s->h_span_in, in_bytes, s->d_span_in, in_bytes, s->d_span, 16 * nn, s->h_span, 16 * nn)) return rc;
    int32_t *h = s->h_span_in.as<int32_t>();
    for (int32_t i = 0; i < n; ++i) {  // (a slot reset since its last chunk has a stale table and no query)
        const int32_t sl = slot[i];
        h[i] = sl;
        h[nn + i] = (!s->raw_fresh[sl] && (s->raw_status[sl] & sfa::kRawCalibrated)) ? static_cast<int32_t>(s->len[sl]) : 0;
        if (per_slot) h[2 * nn + i] = std::max(s->auto_h[sl].skip, 0);  // (a calibrated slot has resolved its skip)
    }
    hipStream_t st = c->stream;
    HIP_TRY(hipMemcpyAsync(s->d_span_in.p, h, in_bytes, hipMemcpyHostToDevice, st));
    sfa::EvSpanArgs a;
    a.slot = s->d_span_in.as<int32_t>();
    a.q_events = a.slot + nn;
    a.events = s->d_evtab.as<sfa::EvRecord>();
    a.span = s->d_span.as<uint64_t>();
    a.n = n;
    a.ev_cap = s->skip + s->query;
    a.skip = s->skip;
    a.query_cap = s->query;
    a.skips = per_slot ? a.slot + 2 * nn : nullptr;
    if (per_slot)
        hipLaunchKernelGGL(sfa::ev_query_span_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL(sfa::ev_query_span_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, st, a);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(s->h_span.p, s->d_span.p, 16 * nn, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "sfa_session_query_span: the gather failed: %s", hipGetErrorString(hipGetLastError()));
    const uint64_t *sp = s->h_span.as<uint64_t>();
    for (int32_t i = 0; i < n; ++i) {
        start_raw[i] = sp[2 * i];
        end_raw[i] = sp[2 * i + 1];
    }
    return SFA_OK;
}

int sfa_session_extend_raw(sfa_session_t *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling,
                           const uint8_t *end_of_read, int32_t n, sfa_result_t *out, sfa_session_raw_info_t *info) {
    if (!s || n < 0 || (n > 0 && (!slot || !raw_off || !scaling || !out || !info))) return fail(SFA_EINVAL, "sfa_session_extend_raw: bad argument");
    if (!s->raw) return fail(SFA_EINVAL, "sfa_session_extend_raw: the session takes events (sfa_session_extend) until sfa_session_raw_config");
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    if (++s->call_no == INT32_MAX) {
        std::fill(s->stamp.begin(), s->stamp.end(), 0);
        s->call_no = 1;
    }
    std::vector<float> scale(2 * static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        if (sl < 0 || sl >= s->n_slots) return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d out of range (the session has %d)", sl, s->n_slots);
        if (s->stamp[sl] == s->call_no) return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d is named twice in one call", sl);
        s->stamp[sl] = s->call_no;
        const int64_t l = raw_off[i + 1] - raw_off[i];
        if (l < 0) return fail(SFA_EINVAL, "sfa_session_extend_raw: raw_off not monotone");
        if (l > 0 && (s->raw_status[sl] & sfa::kRawEnded)) return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d has seen its end of read; it takes no samples until it is reset", sl);
        if (s->raw_n[sl] + l > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_extend_raw: slot %d would hold more than 2^30 samples", sl);
        const double *sc = scaling + 3 * static_cast<size_t>(i);
        if (!s->raw_fresh[sl] && memcmp(sc, &s->raw_scaling[3 * static_cast<size_t>(sl)], 3 * sizeof(double)) != 0)
            return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d: digitisation, offset and range are fixed by a slot's first chunk after a reset", sl);
        const float dig = static_cast<float>(sc[0]), range = static_cast<float>(sc[2]);  // event_single(), src/sigfish.c:343
        scale[2 * static_cast<size_t>(i)] = static_cast<float>(sc[1]);
        scale[2 * static_cast<size_t>(i) + 1] = range / dig;
        if (!std::isfinite(scale[2 * static_cast<size_t>(i)]) || !std::isfinite(scale[2 * static_cast<size_t>(i) + 1]))
            return fail(SFA_EINVAL, "sfa_session_extend_raw: slot %d: the scaling is not finite", sl);
    }
    const int64_t total = raw_off[n] - raw_off[0];
    if (total > INT32_MAX / 2) return fail(SFA_ERANGE, "sfa_session_extend_raw: more than 2^30 samples in one call");
    if (total > 0 && !raw) return fail(SFA_EINVAL, "sfa_session_extend_raw: null samples");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    hipStream_t st = c->stream;

    // entry tables: [raw_off re-based (n + 1) x i64 | slot n x i32 | flags n x i32 | scale 2n x f32]
    const size_t nn = static_cast<size_t>(n);
    const bool auto_on = s->auto_max > 0;
    const size_t o_off = 0, o_slot = align8(8 * (nn + 1)), o_flag = o_slot + align8(4 * nn), o_scale = o_flag + align8(4 * nn);
    // (automatic query start: | have n x i32 | EvAutoEntry n)
    const size_t o_have = o_scale + 8 * nn, o_aent = o_have + align8(4 * nn), bytes = auto_on ? o_aent + sizeof(sfa::EvAutoEntry) * nn : o_have;
    if (int rc = reserve_all(s->h_rstage, bytes, s->d_rstage, bytes, s->d_raw, 2 * static_cast<size_t>(std::max<int64_t>(total, 1)), s->d_rout, sizeof(sfa::EvStreamOut) * nn,
                             s->h_rout, sizeof(sfa::EvStreamOut) * nn, s->d_bad, nn, s->h_bad, nn + 8))
        return rc;
    char *h = s->h_rstage.as<char>();
    const char *d = s->d_rstage.as<char>();
    for (int32_t i = 0; i <= n; ++i) reinterpret_cast<int64_t *>(h + o_off)[i] = raw_off[i] - raw_off[0];
    for (int32_t i = 0; i < n; ++i) {
        reinterpret_cast<int32_t *>(h + o_slot)[i] = slot[i];
        reinterpret_cast<int32_t *>(h + o_flag)[i] = (s->raw_fresh[slot[i]] ? sfa::kEntryFresh : 0) | ((end_of_read && end_of_read[i]) ? sfa::kEntryEnd : 0);
    }
    memcpy(h + o_scale, scale.data(), 8 * nn);
    // automatic query start: the points this call carries every slot past (each slot's count of samples decides, not the calls)
    int32_t n_aent = 0;
    std::vector<int32_t> auto_k_after;
    std::vector<uint8_t> auto_final_now;
    if (auto_on) {
        auto_k_after.assign(nn, 0);
        auto_final_now.assign(nn, 0);
        sfa::EvAutoEntry *ent = reinterpret_cast<sfa::EvAutoEntry *>(h + o_aent);
        const int64_t M = s->auto_max;
        for (int32_t i = 0; i < n; ++i) {
            const int32_t sl = slot[i];
            const int64_t have = s->raw_n[sl], after = have + (raw_off[i + 1] - raw_off[i]);
            reinterpret_cast<int32_t *>(h + o_have)[i] = static_cast<int32_t>(have);
            auto_k_after[i] = s->auto_k[sl];
            if (s->auto_h[sl].target >= 0 || s->auto_final[sl]) continue;  // frozen, or given up: later points are not evaluated
            const int32_t k_hi = s->auto_every > 0 ? static_cast<int32_t>(std::min(after, M) / s->auto_every) : 0;
            const bool ended_now = end_of_read && end_of_read[i] && !(s->raw_status[sl] & sfa::kRawEnded);
            const bool final_now = ended_now || (after >= M && have < M);
            sfa::EvAutoEntry e;
            e.entry = i;
            e.n0 = (s->auto_k[sl] + 1) * s->auto_every;
            e.n_periodic = k_hi - s->auto_k[sl];
            e.n_final = final_now ? static_cast<int32_t>(std::min(after, M)) : -1;
            auto_k_after[i] = k_hi;
            auto_final_now[i] = final_now ? 1 : 0;
            if (e.n_periodic > 0 || final_now) ent[n_aent++] = e;
        }
        if (int rc = reserve_all(s->d_csum, 4 * (static_cast<size_t>(M) + 1) * static_cast<size_t>(std::max(n_aent, 1)), s->d_aout, sizeof(sfa::EvAutoSlot) * nn, s->h_aout,
                                 sizeof(sfa::EvAutoSlot) * nn))
            return rc;
    }
    HIP_TRY(hipMemcpyAsync(s->d_rstage.p, h, bytes, hipMemcpyHostToDevice, st));
    if (total > 0) HIP_TRY(hipMemcpyAsync(s->d_raw.p, raw + raw_off[0], 2 * static_cast<size_t>(total), hipMemcpyHostToDevice, st));

    const bool rna = (c->flag & SFA_RNA) != 0;  // detector parameters, src/events.c:47-58
    sfa::EvStreamArgs ea;
    ea.raw = s->d_raw.as<int16_t>();
    ea.raw_off = reinterpret_cast<const int64_t *>(d + o_off);
    ea.slot = reinterpret_cast<const int32_t *>(d + o_slot);
    ea.e_flags = reinterpret_cast<const int32_t *>(d + o_flag);
    ea.scale = reinterpret_cast<const float *>(d + o_scale);
    ea.state = s->d_state.as<sfa::EvStreamSlot>();
    ea.events = s->d_evtab.as<sfa::EvRecord>();
    ea.n = n;
    ea.ev_cap = s->skip + s->query;
    ea.w1 = rna ? 7 : 3;
    ea.w2 = rna ? 14 : 6;
    ea.thr1 = rna ? 2.5f : 1.4f;
    ea.thr2 = 9.0f;
    ea.peak_height = rna ? 1.0f : 0.2f;
    HIP_TRY(hipEventRecord(s->ev_raw[0], st));
    hipLaunchKernelGGL(sfa::ev_stream_kernel, dim3((n + 63) / 64), dim3(64), 0, st, ea);
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(s->ev_raw[1], st));
    sfa::EvNormArgs na;
    na.slot = ea.slot;
    na.state = ea.state;
    na.window = s->d_window.as<int32_t>();
    na.events = ea.events;
    na.query = s->d_query.as<float>();
    na.out = s->d_rout.as<sfa::EvStreamOut>();
    na.bad = s->d_bad.as<uint8_t>();
    na.n = n;
    na.ev_cap = ea.ev_cap;
    na.skip = s->skip;
    na.norm = s->norm;
    na.query_cap = s->query;
    na.n_at = s->recal_n;
    na.flags = s->recal_flags;
    for (int32_t k = 0; k < sfa::kRecalMaxPoints; ++k) na.at[k] = k < s->recal_n ? s->recal_at[k] : 0;
    na.resweep = s->resweep ? 1 : 0;
    na.reversed = (s->resweep && (c->flag & SFA_RNA) && !(c->flag & SFA_INV)) ? 1 : 0;
    sfa::EvNormAutoArgs nx{nullptr, nullptr};
    if (auto_on) {
        sfa::EvAutoAppendArgs ap;
        ap.raw = ea.raw;
        ap.raw_off = ea.raw_off;
        ap.slot = ea.slot;
        ap.e_flags = ea.e_flags;
        ap.have = reinterpret_cast<const int32_t *>(d + o_have);
        ap.keep = s->d_keep.as<int16_t>();
        ap.state = s->d_auto.as<sfa::EvAutoSlot>();
        ap.n = n;
        ap.max_samples = s->auto_max;
        HIP_TRY(hipEventRecord(s->ev_auto[0], st));
        hipLaunchKernelGGL(sfa::ev_auto_append_kernel, dim3(n), dim3(256), 0, st, ap);
        KERNEL_TRY();
        if (n_aent > 0) {  // slots without a pending point cost nothing
            sfa::EvAutoEvalArgs va;
            va.entries = reinterpret_cast<const sfa::EvAutoEntry *>(d + o_aent);
            va.slot = ea.slot;
            va.scale = ea.scale;
            va.keep = ap.keep;
            va.csum = s->d_csum.as<int32_t>();
            va.state = ap.state;
            va.n_entries = n_aent;
            va.max_samples = s->auto_max;
            va.every = s->auto_every;
            va.lo = c->pore == 2 ? 500 : 2000;  // JNNV2_RNA_RNA004_ADAPTOR / JNNV2_RNA_R9_ADAPTOR, as sfa_align_raw
            va.std_scale = c->pore == 2 ? 0.7f : 0.5f;
            hipLaunchKernelGGL(sfa::ev_auto_eval_kernel, dim3(n_aent), dim3(64), 0, st, va);
            KERNEL_TRY();
        }
        HIP_TRY(hipEventRecord(s->ev_auto[1], st));
        nx.state = ap.state;
        nx.out = s->d_aout.as<sfa::EvAutoSlot>();
        hipLaunchKernelGGL(sfa::ev_stream_norm_kernel<true>, dim3(n), dim3(64), 0, st, na, nx);
        HIP_TRY(hipMemcpyAsync(s->h_aout.p, s->d_aout.p, sizeof(sfa::EvAutoSlot) * nn, hipMemcpyDeviceToHost, st));
    } else {
        hipLaunchKernelGGL(sfa::ev_stream_norm_kernel<false>, dim3(n), dim3(64), 0, st, na, nx);
    }
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(s->ev_raw[2], st));
    // the counts of new events are all that comes back: the planner of the sweep is host code
    HIP_TRY(hipMemcpyAsync(s->h_rout.p, s->d_rout.p, sizeof(sfa::EvStreamOut) * nn, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "sfa_session_extend_raw: the detector failed: %s", hipGetErrorString(hipGetLastError()));

    const sfa::EvStreamOut *ro = s->h_rout.as<sfa::EvStreamOut>();
    std::vector<Chunk> ch(n);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        if (s->raw_fresh[sl]) memcpy(&s->raw_scaling[3 * static_cast<size_t>(sl)], scaling + 3 * static_cast<size_t>(i), 3 * sizeof(double));
        s->raw_fresh[sl] = 0;
        s->raw_n[sl] += raw_off[i + 1] - raw_off[i];
        s->raw_nev[sl] = ro[i].n_events;
        s->raw_status[sl] = ro[i].status & 15;
        s->raw_mean[sl] = ro[i].mean;
        s->raw_sd[sl] = ro[i].sd;
        s->raw_window[sl] = ro[i].window;
        if (auto_on) {
            s->auto_h[sl] = s->h_aout.as<sfa::EvAutoSlot>()[i];
            s->auto_k[sl] = auto_k_after[i];
            s->auto_final[sl] |= auto_final_now[i];
        }
        // a recalibrated slot: its whole query was rewritten, so it is swept as a first chunk, which reads no carried row and
        // writes a new one (the planner never puts first and carried chunks into one wave).  A resweep session knows no other
        // sweep: q_new is the window then, and 0 in every call that leaves the window as it is
        if (ro[i].q_new > 0 && ro[i].q_first == 0) s->len[sl] = 0;
        ch[i] = Chunk{static_cast<int64_t>(sl) * s->query + ro[i].q_first, ro[i].q_new};
    }
    float t_ev = 0, t_norm = 0;
    HIP_TRY(hipEventElapsedTime(&t_ev, s->ev_raw[0], s->ev_raw[1]));
    HIP_TRY(hipEventElapsedTime(&t_norm, s->ev_raw[1], s->ev_raw[2]));
    if (auto_on) {
        float t_auto = 0;
        HIP_TRY(hipEventElapsedTime(&t_auto, s->ev_auto[0], s->ev_auto[1]));
        s->auto_ms = t_auto;
    }
    if (int rc = sweep_chunks(s, slot, ch.data(), n, nullptr, 0, s->d_query.as<float>(), out)) return rc;
    c->prof.events_ms = t_ev;
    c->prof.normalise_ms = t_norm;
    c->prof.total_ms += t_ev + t_norm;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t sl = slot[i];
        sfa_session_raw_info_t &f = info[i];
        f.n_samples = s->raw_n[sl];
        f.n_events = s->raw_nev[sl];
        f.q_events = s->len[sl];
        f.norm_mean = s->raw_mean[sl];
        f.norm_sd = s->raw_sd[sl];
        f.status = s->raw_status[sl] | (ro[i].status & sfa::kRawResweep);
        f.norm_window = s->raw_window[sl];
    }
    return SFA_OK;
}

}  // extern "C"
