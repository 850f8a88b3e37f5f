// sfa_session_targets.hip -- what a session knows about the reference beside its rows, and the calls that read a slot's carried
// row with it (include/sigfish_amd.h): targets and their classes (target_rules.hpp), target groups (group_rules.hpp), open and
// closed groups (quota_rules.hpp), the two depth caps (coverage_rules.hpp, group_cover_rules.hpp) and the two reach lists
// (reach_rules.hpp, reach_group_rules.hpp).  The kernels are the sdtw_inst_session_* units'; this unit has no device code.
// Stated once here, for every entry point of the family:
//   the refusals of a configuration call      refuse_resweep, refuse_wide
//   the reference as the host rules read it   HostModel, ref_columns
//   what goes with what when a feature goes   targets_off, groups_off (and the two caps' mask_cap_off, group_cap_off)
//   a query call, stage by stage              query_run; on a spread session spread_query
#include "sfa_session_state.hpp"

namespace {

// ---- what the configuration calls refuse, and the reference as the host rules read it ----

int refuse_resweep(const sfa_session *s, const char *who) {
    if (!s->resweep) return SFA_OK;
    return fail(SFA_EINVAL, "%s: the session was created with SFA_SESSION_RESWEEP: its carried row belongs to the reversed query, and what its minimum means has "
                            "not been looked into",
                who);
}

// (`what` counts the columns: "classes" or "groups")
int refuse_wide(const sfa_ctx *c, const char *who, const char *what) {
    if (c->model.total_cols < INT32_MAX) return SFA_OK;
    return fail(SFA_ERANGE, "%s: the reference has %lld columns; the %s count them in 31 bits", who, (long long)c->model.total_cols, what);
}

// the session whose state says what is configured: of a spread session sub-session 0, which always exists (spread_create refuses
// n_slots <= 0, and shard 0 holds slot 0); every sub-session holds the same masks, tables and tracks
sfa_session *state_of(sfa_session *s) { return s->spread ? s->spread->subs[0] : s; }

// the reference model as the host rules read it (host tables; jobs are contig-major, '+' before '-': sfa_context.hip)
struct HostModel {
    std::vector<int32_t> job_contig, ref_len;
    std::vector<int8_t> job_strand;
    sfa::TargetModel m;
    HostModel(const sfa_session *s) {
        const sfa_ctx *c = s->c;
        const int32_t nj = c->model.n_jobs, strands = nj / c->model.num_ref;
        job_contig.resize(nj), job_strand.resize(nj), ref_len.resize(c->model.num_ref);
        for (int32_t j = 0; j < nj; ++j) job_contig[j] = j / strands, job_strand[j] = (j % strands) ? '-' : '+';
        for (int32_t r = 0; r < c->model.num_ref; ++r) ref_len[r] = c->model.h_job_len[static_cast<size_t>(r) * strands];
        m = sfa::TargetModel{c->model.num_ref, nj, job_contig.data(), job_strand.data(), c->model.h_job_len.data(), s->rows.h_col_off.data(), ref_len.data(),
                             c->model.h_ref_off.data(), c->model.total_cols};
    }
};

// a reference before any context exists (the *_bytes functions): the columns of a slot's row, the entries of the depth tracks;
// false: not a reference
bool ref_columns(const sfa_ref_t *ref, int flag, int64_t *entries, int64_t *cols) {
    if (!ref || ref->num_ref <= 0 || !ref->ref_lengths) return false;
    *entries = *cols = 0;
    for (int32_t r = 0; r < ref->num_ref; ++r) {
        if (ref->ref_lengths[r] <= 0) return false;
        *entries += sfa::coverage_track_len(ref->ref_lengths[r]);
        *cols += static_cast<int64_t>(ref->ref_lengths[r]) * ((flag & SFA_RNA) ? 1 : 2);
    }
    return true;
}

// ---- what goes with what when something is switched off.  Host statements only: the caller has synchronised the stream ----

// a cap goes; the session's one depth track goes with the last of the two
void mask_cap_off(sfa_session *s) {
    s->cover.free_mask();
    if (!s->gcover.on()) s->cover.free_track();
}
void group_cap_off(sfa_session *s) {
    s->gcover.free_all();
    if (!s->cover.on()) s->cover.free_track();
}
// the mask goes: a reach list's anchors and the mask's cap, which lives on it, go with it (the buffers of a query call stay for
// the next mask)
void targets_off(sfa_session *s) {
    sess::Targets &t = s->targets;
    t.on = false;
    t.on_cols = 0;
    t.first_on = t.first_off = -1;
    std::vector<uint32_t>().swap(t.h_mask);
    t.d_mask = DevBuf{};
    s->reach.free_all();
    mask_cap_off(s);
}
// the labels go: a reach list's anchors, the group cap, which lives on them, and the labels' first columns go with them
void groups_off(sfa_session *s) {
    sess::Groups &g = s->groups;
    g.n_groups = 0;
    std::vector<uint16_t>().swap(g.h_label);
    g.d_label = DevBuf{};
    s->open.first.clear();
    s->greach.free_all();
    group_cap_off(s);
}
// A reach list that failed half-way.  Its build overwrites the old mask / table, so an allocation or device failure leaves the
// session without the feature -- and so without the cap that lives on it -- never with half of two lists (include/sigfish_amd.h
// says so).  The code and the message stay those of the failure
int targets_give_up(sfa_session *s, int rc) {
    (void)hipStreamSynchronize(s->c->stream);
    targets_off(s);
    return rc;
}
int groups_give_up(sfa_session *s, int rc) {
    (void)hipStreamSynchronize(s->c->stream);
    groups_off(s);
    return rc;
}

// ---- the live mask and the live label table of the caps ----

void take_stats(const sfa::CoverStats &st, int64_t *cols, int32_t *first_on, int32_t *first_off) {
    *cols = static_cast<int64_t>(st.live);
    *first_on = st.first_on == sfa::kNoColumn ? -1 : st.first_on;
    *first_off = st.first_off == sfa::kNoColumn ? -1 : st.first_off;
}

// the argument block of session_cover_mask_kernel, and of session_reach_live_kernel but for its anchors
template <class A>
A cover_mask_args(const sfa_session *s) {
    const sfa_ctx *c = s->c;
    const sess::Coverage &v = s->cover;
    A a;
    a.base = s->targets.d_mask.as<uint32_t>();
    a.live = v.d_live.as<uint32_t>();
    a.depth = v.d_depth.as<uint32_t>();
    a.cov_off = v.d_cov_off.as<int64_t>();
    a.col_off = s->rows.d_col_off.as<int64_t>();
    a.ref = c->model.tables();
    a.stats = v.d_stats.as<sfa::CoverStats>();
    a.total_cols = c->model.total_cols;
    a.n_jobs = c->model.n_jobs;
    a.n_words = static_cast<int32_t>(sfa::target_mask_words(c->model.total_cols));
    a.cap = static_cast<uint32_t>(v.cap);
    return a;
}

// The live mask from the base mask and the depth tracks (session_cover_mask_kernel; on a reach session session_reach_live_kernel,
// which reads the depth at the column's anchor), on the context's stream; the caller has set the device and synchronises.  The
// upload in front resets the record the kernel's atomics merge into.
int cover_enqueue_mask(sfa_session *s) {
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    sfa::CoverStats *hs = v.h_stats.as<sfa::CoverStats>();
    hs[0] = sfa::CoverStats{0ull, sfa::kNoColumn, sfa::kNoColumn};
    HIP_TRY(hipMemcpyAsync(v.d_stats.p, hs, sizeof(sfa::CoverStats), hipMemcpyHostToDevice, c->stream));
    const dim3 grid(sfa::cover_mask_blocks(c->model.total_cols)), block(sfa::kCoverThreads);
    if (s->reach.on) {
        auto a = cover_mask_args<sfa::SessionReachLiveArgs>(s);
        a.anchor = s->reach.d_anchor.as<int32_t>();
        hipLaunchKernelGGL(sfa::session_reach_live_kernel, grid, block, 0, c->stream, a);
    } else {
        hipLaunchKernelGGL(sfa::session_cover_mask_kernel, grid, block, 0, c->stream, cover_mask_args<sfa::SessionCoverMaskArgs>(s));
    }
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(hs + 1, v.d_stats.p, sizeof(sfa::CoverStats), hipMemcpyDeviceToHost, c->stream));
    return SFA_OK;
}
// ... and what it left, once the stream is through
void cover_collect(sfa_session *s) {
    sess::Coverage &v = s->cover;
    take_stats(v.h_stats.as<sfa::CoverStats>()[1], &v.live_cols, &v.first_on, &v.first_off);
}
int cover_derive(sfa_session *s, const char *who) {
    if (int rc = cover_enqueue_mask(s)) return rc;
    if (hipStreamSynchronize(s->c->stream) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    cover_collect(s);
    return SFA_OK;
}

// what the four kernels over the label table and the depth tracks share of their argument blocks: session_cover_label_kernel and
// session_cover_group_kernel, and with anchors session_reach_label_live_kernel and session_reach_label_group_kernel
template <class A>
A group_cover_args(const sfa_session *s) {
    const sfa_ctx *c = s->c;
    A a;
    a.base = s->groups.d_label.as<uint64_t>();
    a.depth = s->cover.d_depth.as<uint32_t>();
    a.cov_off = s->cover.d_cov_off.as<int64_t>();
    a.col_off = s->rows.d_col_off.as<int64_t>();
    a.ref = c->model.tables();
    a.total_cols = c->model.total_cols;
    a.n_jobs = c->model.n_jobs;
    a.n_groups = s->groups.n_groups;
    a.cap = static_cast<uint32_t>(s->gcover.cap);
    return a;
}
template <class A>
A cover_label_args(const sfa_session *s) {
    A a = group_cover_args<A>(s);
    a.live = s->gcover.d_live.as<uint16_t>();
    a.first = s->gcover.d_first.as<int32_t>();
    return a;
}

// The live label table from the base table and the depth tracks (session_cover_label_kernel; on a reach label table
// session_reach_label_live_kernel, which reads the depth at the column's anchor), on the context's stream; the caller has set the
// device and synchronises.  The upload in front resets the table of firsts the kernel's atomics merge into.
int gcover_enqueue_labels(sfa_session *s) {
    sfa_ctx *c = s->c;
    sess::GroupCover &gc = s->gcover;
    const size_t entries = static_cast<size_t>(s->groups.n_groups) + 1;
    int32_t *hf = gc.h_first.as<int32_t>();
    std::fill(hf, hf + entries, sfa::kNoColumn);
    HIP_TRY(hipMemcpyAsync(gc.d_first.p, hf, 4 * entries, hipMemcpyHostToDevice, c->stream));
    const dim3 grid(sfa::group_cover_blocks(c->model.total_cols)), block(sfa::kGroupCoverThreads);
    if (s->greach.on) {
        auto a = cover_label_args<sfa::SessionReachLabelLiveArgs>(s);
        a.anchor = s->greach.d_anchor.as<int32_t>();
        hipLaunchKernelGGL(sfa::session_reach_label_live_kernel, grid, block, 0, c->stream, a);
    } else {
        hipLaunchKernelGGL(sfa::session_cover_label_kernel, grid, block, 0, c->stream, cover_label_args<sfa::SessionCoverLabelArgs>(s));
    }
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(hf + entries, gc.d_first.p, 4 * entries, hipMemcpyDeviceToHost, c->stream));
    return SFA_OK;
}
// ... and what it left, once the stream is through
void gcover_collect(sfa_session *s) {
    sess::GroupCover &gc = s->gcover;
    sfa::group_cover_firsts_for_open(gc.h_first.as<int32_t>() + s->groups.n_groups + 1, s->groups.n_groups, &gc.first);
}
// the whole live table anew: the base table's bytes (the words behind the row with them), then the derive
int gcover_derive(sfa_session *s, const char *who) {
    sfa_ctx *c = s->c;
    HIP_TRY(hipMemcpyAsync(s->gcover.d_live.p, s->groups.d_label.p, 8 * sfa::group_label_words(c->model.total_cols), hipMemcpyDeviceToDevice, c->stream));
    if (int rc = gcover_enqueue_labels(s)) return rc;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    gcover_collect(s);
    return SFA_OK;
}

// The session's one depth track, for whichever cap is configured: reserved and its offsets uploaded, and zeroed when `zero` (the
// caller's: the other cap is off, so nobody's depth is lost).  The caller has set the device; the stream is idle.
int cover_track_up(sfa_session *s, const bool zero) {
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    const HostModel hm(s);
    std::vector<int64_t> cov_off;
    sfa::coverage_offsets(hm.ref_len.data(), c->model.num_ref, &cov_off);
    const bool fresh = !v.has_track();
    if (int rc = v.reserve_track(cov_off.back(), c->model.num_ref)) return rc;
    if (int rc = sess::create_events(v.ev, 2)) return rc;
    v.h_cov_off.swap(cov_off);
    HIP_TRY(hipMemcpyAsync(v.d_cov_off.p, v.h_cov_off.data(), 8 * v.h_cov_off.size(), hipMemcpyHostToDevice, c->stream));
    if (zero || fresh) HIP_TRY(hipMemsetAsync(v.d_depth.p, 0, 4 * static_cast<size_t>(v.h_cov_off.back()), c->stream));
    return SFA_OK;
}

// ---- the builds of the two reach lists.  The caller has set the device and synchronised; from the first statement on the old
// mask / table is gone, so whatever fails here the caller gives the feature up (targets_give_up, groups_give_up) ----

// the mask and its anchors from the prepared runs (session_reach_build_kernel)
int reach_build(sfa_session *s, const sfa::ReachPrepared &prep, const char *who) {
    sfa_ctx *c = s->c;
    sess::Targets &t = s->targets;
    sess::Reach &r = s->reach;
    if (int rc = t.reserve(c->model.total_cols)) return rc;
    if (int rc = r.reserve(c->model.total_cols, prep.runs.size(), c->model.n_jobs)) return rc;
    hipStream_t st = c->stream;
    const size_t words = sfa::target_mask_words(c->model.total_cols);
    sfa::CoverStats *hs = r.h_stats.as<sfa::CoverStats>();
    hs[0] = sfa::CoverStats{0ull, sfa::kNoColumn, sfa::kNoColumn};
    sfa::SessionReachBuildArgs a;
    a.runs = r.d_runs.as<sfa::ReachRun>();
    a.run_off = r.d_run_off.as<int32_t>();
    a.col_off = s->rows.d_col_off.as<int64_t>();
    a.mask = t.d_mask.as<uint32_t>();
    a.anchor = r.d_anchor.as<int32_t>();
    a.stats = r.d_stats.as<sfa::CoverStats>();
    a.total_cols = c->model.total_cols;
    a.n_jobs = c->model.n_jobs;
    a.n_words = static_cast<int32_t>(words);
    // (the uploads of the runs read pageable memory: they are through when the calls return)
    HIP_TRY(hipMemcpyAsync(r.d_stats.p, hs, sizeof(sfa::CoverStats), hipMemcpyHostToDevice, st));
    if (!prep.runs.empty()) HIP_TRY(hipMemcpyAsync(r.d_runs.p, prep.runs.data(), sizeof(sfa::ReachRun) * prep.runs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(r.d_run_off.p, prep.run_off.data(), 4 * prep.run_off.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(t.d_mask.p, 0, 4 * words, st));  // (the spare word stays zero)
    hipLaunchKernelGGL(sfa::session_reach_build_kernel, dim3(sfa::cover_mask_blocks(c->model.total_cols)), dim3(sfa::kCoverThreads), 0, st, a);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(hs + 1, r.d_stats.p, sizeof(sfa::CoverStats), hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    r.d_runs = DevBuf{}, r.d_run_off = DevBuf{};  // (the runs were the call's: only the anchors and the 16-byte record stay)
    std::vector<uint32_t>().swap(t.h_mask);  // (the mask was built on the device: sfa_session_reach_tables copies it back)
    take_stats(hs[1], &t.on_cols, &t.first_on, &t.first_off);
    t.on = true;
    r.on = true;
    return SFA_OK;
}

// the label table and its anchors from the prepared runs (session_reach_label_build_kernel)
int reach_group_build(sfa_session *s, const sfa::ReachGroupPrepared &prep, int32_t n_groups, const char *who) {
    sfa_ctx *c = s->c;
    sess::Groups &g = s->groups;
    sess::GroupReach &gr = s->greach;
    s->open.first.clear();
    g.n_groups = 0;  // (off until the new table is up)
    std::vector<uint16_t>().swap(g.h_label);  // (the table is built on the device: sfa_session_group_reach_tables copies it back)
    gr.on = false;
    if (int rc = g.reserve(c->model.total_cols)) return rc;
    if (int rc = gr.reserve(c->model.total_cols, prep.runs.size(), c->model.n_jobs, n_groups)) return rc;
    if (s->gcover.on())  // (the live table's tables follow the new n_groups)
        if (int rc = s->gcover.reserve(c->model.total_cols, n_groups)) return rc;
    hipStream_t st = c->stream;
    const size_t entries = static_cast<size_t>(n_groups) + 1;
    int32_t *hf = gr.h_first.as<int32_t>();
    std::fill(hf, hf + entries, sfa::kNoColumn);
    sfa::SessionReachLabelBuildArgs a;
    a.runs = gr.d_runs.as<sfa::ReachGroupRun>();
    a.run_off = gr.d_run_off.as<int32_t>();
    a.col_off = s->rows.d_col_off.as<int64_t>();
    a.label = g.d_label.as<uint16_t>();
    a.anchor = gr.d_anchor.as<int32_t>();
    a.first = gr.d_first.as<int32_t>();
    a.total_cols = c->model.total_cols;
    a.n_jobs = c->model.n_jobs;
    a.n_groups = n_groups;
    // the labels from the row's last quad on, the word behind the row with them: the background (the kernel writes the row's own)
    const size_t tail = 4 * static_cast<size_t>(c->model.total_cols / 4), n_tail = 4 * sfa::group_label_words(c->model.total_cols) - tail;
    // (the uploads of the runs read pageable memory: they are through when the calls return)
    HIP_TRY(hipMemcpyAsync(gr.d_first.p, hf, 4 * entries, hipMemcpyHostToDevice, st));
    if (!prep.runs.empty()) HIP_TRY(hipMemcpyAsync(gr.d_runs.p, prep.runs.data(), sizeof(sfa::ReachGroupRun) * prep.runs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(gr.d_run_off.p, prep.run_off.data(), 4 * prep.run_off.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(g.d_label.as<uint16_t>() + tail), static_cast<unsigned short>(n_groups), n_tail, st));
    hipLaunchKernelGGL(sfa::session_reach_label_build_kernel, dim3(sfa::group_cover_blocks(c->model.total_cols)), dim3(sfa::kGroupCoverThreads), 0, st, a);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(hf + entries, gr.d_first.p, 4 * entries, hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    sfa::group_cover_firsts_for_open(hf + entries, n_groups, &s->open.first);  // (what sfa_session_open_classes needs once per label table)
    gr.free_call();  // (the runs and the firsts were the call's: only the anchors stay)
    g.n_groups = n_groups;
    gr.on = true;
    return SFA_OK;
}

// ---- the query calls: sfa_session_classes, sfa_session_group_bests, sfa_session_open_classes ----
// A call supplies Q: reserve(m, parts), its buffers; none(), the record of an entry that is not launched, into every one of the
// caller's; fill(m, parts), its two argument blocks; launch(m, parts, stream), its two kernels and what must lie in front of them;
// copy_back(m, stream); scatter(k, i, n_events), launched entry k into the caller's entry i.  Its own refusals ("the feature is
// off", a bitmap of the wrong size) come in front of query_run.  Then, in this order and for all three: a slot out of range, a
// slot named twice, n == 0 (nothing is done), a batch submitted and never waited for (its error words are this call's), more
// blocks than a launch takes, memory.  Every refusal comes before the first write to the caller's records.
template <class Q>
int query_run(sfa_session *s, const int32_t *slot, int32_t n, const char *who, Q &q) {
    if (int rc = check_slots(s, slot, n, who)) return rc;
    begin_call(s);  // (the stamps say which slots this call has named)
    for (int32_t i = 0; i < n; ++i)
        if (int rc = claim_slot(s, slot[i], who)) return rc;
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    sess::Query &qs = s->query;
    sfa::query_live_entries(slot, n, s->rows.poison.data(), s->rows.len.data(), &qs.live);  // empty and poisoned slots are not launched
    const int32_t m = static_cast<int32_t>(qs.live.size()), parts = sfa::class_parts(c->model.total_cols);
    if (!sfa::query_blocks_fit(m, parts)) return fail(SFA_ERANGE, "%s: %d slots x %d parts of a row are more blocks than a launch takes", who, m, parts);
    if (m > 0) {
        if (int rc = qs.reserve(static_cast<size_t>(m))) return rc;
        if (int rc = q.reserve(static_cast<size_t>(m), static_cast<size_t>(parts))) return rc;
    }
    q.none();
    float ms = 0;
    if (m > 0) {
        int32_t *hs = qs.h_slot.as<int32_t>();
        sfa::query_live_slots(slot, qs.live, hs);
        hipStream_t st = c->stream;
        HIP_TRY(hipMemcpyAsync(qs.d_slot.p, hs, 4 * static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        q.fill(m, parts);
        HIP_TRY(hipEventRecord(qs.ev[0], st));
        if (int rc = q.launch(m, parts, st)) return rc;
        HIP_TRY(hipEventRecord(qs.ev[1], st));
        if (int rc = q.copy_back(m, st)) return rc;
        if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
        HIP_TRY(hipEventElapsedTime(&ms, qs.ev[0], qs.ev[1]));
        sfa::query_scatter(slot, qs.live, [&](int32_t k, int32_t i, int32_t sl) { q.scatter(k, i, static_cast<int32_t>(s->rows.len[sl])); });
    }
    call_profile(c, ms);
    return SFA_OK;
}

// The same call on a spread session: dealt to the shards (a slot is named once); every shard that has entries runs fn(its
// sub-session, its part of the call, its buffers) -- resize the buffer, call the sub-session, scatter -- and the others idle, so
// that the group's profile is this call's on every shard
template <typename F>
int spread_query(sfa_session *s, const int32_t *slot, int32_t n, const char *who, F fn) {
    if (int rc = spread_deal(s, slot, n, true, who)) return rc;
    return sfa::for_each_shard(s->c, [&](size_t r) {
        const sfa::SpreadShardPart &p = s->spread->part.shard[r];
        return p.n() == 0 ? spread_idle(s->c->shards[r]) : fn(s->spread->subs[r], p, s->spread->shard[r]);
    });
}

struct ClassQuery {  // sfa_session_classes (sdtw_session_class.hpp)
    sfa_session *s;
    sfa_class_t *out;
    int32_t n;
    sfa::SessionClassArgs a;
    sfa::SessionClassRowsArgs ra;
    int reserve(size_t m, size_t parts) { return s->targets.reserve_call(m, parts); }
    void none() {
        sfa_class_t no_class{};
        no_class.on_score = no_class.off_score = INFINITY;
        no_class.on_rid = no_class.on_pos_end = no_class.off_rid = no_class.off_pos_end = -1;
        for (int32_t i = 0; i < n; ++i) out[i] = no_class;
    }
    void fill(int32_t m, int32_t parts) {
        const sfa_ctx *c = s->c;
        const sess::Targets &t = s->targets;
        const bool capped = s->cover.on();  // (the live mask and its firsts: the kernel is the same, another pointer)
        a.slot = s->query.d_slot.as<int32_t>();
        a.rows = s->rows.d_row_c.as<float>() + sfa::kSessionPad;
        a.mask = capped ? s->cover.d_live.as<uint32_t>() : t.d_mask.as<uint32_t>();
        a.part = t.d_part.as<sfa::ClassPartial>();
        a.total_cols = c->model.total_cols;
        a.n = m;
        a.n_parts = parts;
        ra.part = a.part;
        ra.col_off = s->rows.d_col_off.as<int64_t>();
        ra.ref = c->model.tables();
        ra.out = t.d_cls.as<sfa_class_t>();
        ra.n = m;
        ra.n_parts = parts;
        ra.n_jobs = c->model.n_jobs;
        ra.first_on = capped ? s->cover.first_on : t.first_on;
        ra.first_off = capped ? s->cover.first_off : t.first_off;
    }
    int launch(int32_t m, int32_t parts, hipStream_t st) {
        hipLaunchKernelGGL(sfa::sdtw_session_class_kernel, dim3(static_cast<unsigned>(m) * parts), dim3(sfa::kClassThreads), 0, st, a);
        KERNEL_TRY();
        hipLaunchKernelGGL(sfa::sdtw_session_class_rows_kernel, dim3(m), dim3(64), 0, st, ra);
        KERNEL_TRY();
        return SFA_OK;
    }
    int copy_back(int32_t m, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(s->targets.h_cls.p, s->targets.d_cls.p, sizeof(sfa_class_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        return SFA_OK;
    }
    void scatter(int32_t k, int32_t i, int32_t n_events) {
        out[i] = s->targets.h_cls.as<sfa_class_t>()[k];
        out[i].n_events = n_events;
    }
};

struct GroupQuery {  // sfa_session_group_bests (sdtw_session_group.hpp); bests may be null
    sfa_session *s;
    sfa_group_best_t *bests;
    sfa_group_head_t *heads;
    int32_t n;
    sfa::SessionGroupArgs a;
    sfa::SessionGroupRowsArgs ra;
    size_t entries() const { return static_cast<size_t>(s->groups.n_groups) + 1; }
    int reserve(size_t m, size_t) { return s->groups.reserve_call(m, entries(), bests != nullptr); }
    void none() {
        sfa_group_best_t no_best{};
        no_best.score = INFINITY;
        no_best.rid = no_best.pos_end = -1;
        for (int32_t i = 0; i < n; ++i) heads[i] = sfa::group_head_none();
        if (bests)
            for (size_t k = 0; k < static_cast<size_t>(n) * entries(); ++k) bests[k] = no_best;
    }
    void fill(int32_t m, int32_t parts) {
        const sfa_ctx *c = s->c;
        const sess::Groups &g = s->groups;
        a.slot = s->query.d_slot.as<int32_t>();
        a.rows = s->rows.d_row_c.as<float>() + sfa::kSessionPad;
        a.label = s->gcover.on() ? s->gcover.d_live.as<uint64_t>() : g.d_label.as<uint64_t>();  // (the kernel is the same: another pointer)
        a.key = g.d_key.as<unsigned long long>();
        a.total_cols = c->model.total_cols;
        a.n = m;
        a.n_parts = parts;
        a.n_entries = static_cast<int32_t>(entries());
        ra.key = a.key;
        ra.col_off = s->rows.d_col_off.as<int64_t>();
        ra.ref = c->model.tables();
        ra.best = bests ? g.d_best.as<sfa_group_best_t>() : nullptr;
        ra.head = g.d_head.as<sfa_group_head_t>();
        ra.n = m;
        ra.n_entries = a.n_entries;
        ra.n_jobs = c->model.n_jobs;
    }
    int launch(int32_t m, int32_t parts, hipStream_t st) {
        HIP_TRY(hipMemsetAsync(s->groups.d_key.p, 0xff, 8 * static_cast<size_t>(m) * entries(), st));  // all-ones: no column met
        hipLaunchKernelGGL(sfa::sdtw_session_group_kernel, dim3(static_cast<unsigned>(m) * parts), dim3(sfa::kClassThreads), 0, st, a);
        KERNEL_TRY();
        hipLaunchKernelGGL(sfa::sdtw_session_group_rows_kernel, dim3(m), dim3(64), 0, st, ra);
        KERNEL_TRY();
        return SFA_OK;
    }
    int copy_back(int32_t m, hipStream_t st) {
        const sess::Groups &g = s->groups;
        HIP_TRY(hipMemcpyAsync(g.h_head.p, g.d_head.p, sizeof(sfa_group_head_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        if (bests) HIP_TRY(hipMemcpyAsync(g.h_best.p, g.d_best.p, sizeof(sfa_group_best_t) * static_cast<size_t>(m) * entries(), hipMemcpyDeviceToHost, st));
        return SFA_OK;
    }
    void scatter(int32_t k, int32_t i, int32_t n_events) {
        heads[i] = s->groups.h_head.as<sfa_group_head_t>()[k];
        heads[i].n_events = n_events;
        if (bests) memcpy(bests + static_cast<size_t>(i) * entries(), s->groups.h_best.as<sfa_group_best_t>() + static_cast<size_t>(k) * entries(), sizeof(sfa_group_best_t) * entries());
    }
};

struct OpenQuery {  // sfa_session_open_classes (sdtw_session_open.hpp); open may be null: every group is open
    sfa_session *s;
    const uint32_t *open;
    sfa_open_class_t *out;
    int32_t n;
    sfa::SessionOpenArgs a;
    sfa::SessionOpenRowsArgs ra;
    int reserve(size_t m, size_t parts) { return s->open.reserve(m, parts); }
    void none() {
        for (int32_t i = 0; i < n; ++i) out[i] = sfa::open_class_none();
    }
    void fill(int32_t m, int32_t parts) {
        const sfa_ctx *c = s->c;
        const sess::Groups &g = s->groups;
        sess::Open &o = s->open;
        const bool capped = s->gcover.on();  // (the live table and its firsts, which the derive left: the kernels are the same)
        if (!capped && o.first.empty()) sfa::open_label_firsts(g.h_label.data(), c->model.total_cols, g.n_groups, &o.first);
        a.slot = s->query.d_slot.as<int32_t>();
        a.rows = s->rows.d_row_c.as<float>() + sfa::kSessionPad;
        a.label = capped ? s->gcover.d_live.as<uint64_t>() : g.d_label.as<uint64_t>();
        a.part = o.d_part.as<sfa::ClassPartial>();
        a.total_cols = c->model.total_cols;
        a.n = m;
        a.n_parts = parts;
        sfa::open_normalise(open, g.n_groups, a.open);  // (the bitmap travels in the argument block: nothing is uploaded)
        ra.part = a.part;
        ra.col_off = s->rows.d_col_off.as<int64_t>();
        ra.ref = c->model.tables();
        ra.label = capped ? s->gcover.d_live.as<uint16_t>() : g.d_label.as<uint16_t>();
        ra.out = o.d_out.as<sfa_open_class_t>();
        ra.n = m;
        ra.n_parts = parts;
        ra.n_jobs = c->model.n_jobs;
        sfa::open_first_cols(capped ? s->gcover.first : o.first, g.n_groups, a.open, &ra.first_on, &ra.first_off);
    }
    int launch(int32_t m, int32_t parts, hipStream_t st) {
        hipLaunchKernelGGL(sfa::sdtw_session_open_kernel, dim3(static_cast<unsigned>(m) * parts), dim3(sfa::kClassThreads), 0, st, a);
        KERNEL_TRY();
        hipLaunchKernelGGL(sfa::sdtw_session_open_rows_kernel, dim3(m), dim3(64), 0, st, ra);
        KERNEL_TRY();
        return SFA_OK;
    }
    int copy_back(int32_t m, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(s->open.h_out.p, s->open.d_out.p, sizeof(sfa_open_class_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        return SFA_OK;
    }
    void scatter(int32_t k, int32_t i, int32_t n_events) {
        out[i] = s->open.h_out.as<sfa_open_class_t>()[k];
        out[i].cls.n_events = n_events;
    }
};

}  // namespace

extern "C" {

// ---- target classes (target_rules.hpp, sdtw_session_class.hpp) ----

int sfa_session_targets(sfa_session_t *s, const sfa_target_t *targets, int32_t n) {
    static const char *const who = "sfa_session_targets";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = refuse_resweep(s, who)) return rc;
    // (every sub-session holds the mask; no slot needs to be empty, so this is spread_all, not spread_config)
    if (s->spread) return spread_all(s, who, [&](sfa_session *sub) { return sfa_session_targets(sub, targets, n); });
    sfa_ctx *c = s->c;
    sess::Targets &t = s->targets;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a mask in use is not replaced under a kernel)
    if (n == 0) {
        targets_off(s);
        return SFA_OK;
    }
    if (int rc = refuse_wide(c, who, "classes")) return rc;
    const HostModel hm(s);
    char msg[192];
    if (sfa::target_list_error(targets, n, hm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    std::vector<uint32_t> mask;
    const int64_t on_cols = sfa::target_mask(targets, n, hm.m, &mask);
    if (int rc = t.reserve(c->model.total_cols)) return rc;
    s->reach.free_all();  // (a plain mask replaces a reach list, before the mask is overwritten: no anchor outlives the mask it belongs to)
    t.h_mask.swap(mask);
    HIP_TRY(hipMemcpyAsync(t.d_mask.p, t.h_mask.data(), 4 * t.h_mask.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    t.on_cols = on_cols;
    t.first_on = sfa::target_first_of_class(t.h_mask, c->model.total_cols, true);
    t.first_off = sfa::target_first_of_class(t.h_mask, c->model.total_cols, false);
    t.on = true;
    if (s->cover.on()) return cover_derive(s, who);  // (the depth is kept: the live mask of the new base mask, read at the column's own coordinate)
    return SFA_OK;
}

int64_t sfa_session_target_columns(sfa_session_t *s) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_target_columns: null session");
    s = state_of(s);
    if (s->cover.on()) return s->cover.live_cols;
    return s->targets.on ? s->targets.on_cols : 0;
}

int sfa_session_classes(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_class_t *out) {
    static const char *const who = "sfa_session_classes";
    if (!s || n < 0 || (n > 0 && (!slot || !out))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = spread_live(s, who)) return rc;
    if (!state_of(s)->targets.on) return fail(SFA_EINVAL, "%s: the session has no targets (sfa_session_targets)", who);
    if (s->spread)
        return spread_query(s, slot, n, who, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
            b.cls.resize(p.local.size());
            if (int rc = sfa_session_classes(sub, p.local.data(), p.n(), b.cls.data())) return rc;
            sfa::spread_scatter(p, b.cls.data(), out);
            return static_cast<int>(SFA_OK);
        });
    ClassQuery q{s, out, n};
    return query_run(s, slot, n, who, q);
}

int sfa_target_decide(const sfa_class_t *cls, int32_t mode, int32_t min_events, float margin) {
    return cls ? sfa::target_decide(*cls, mode, min_events, margin) : 0;
}

// ---- reach targets (reach_rules.hpp, sdtw_session_reach.hpp) ----

size_t sfa_session_reach_bytes(const sfa_ref_t *ref, int flag) {
    int64_t entries = 0, cols = 0;
    return ref_columns(ref, flag, &entries, &cols) ? sfa::reach_bytes(cols) : 0;
}

int sfa_session_targets_reach(sfa_session_t *s, const sfa_reach_target_t *targets, int32_t n) {
    static const char *const who = "sfa_session_targets_reach";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = refuse_resweep(s, who)) return rc;
    if (n == 0) return sfa_session_targets(s, nullptr, 0);  // (targets off, the anchors freed: one path)
    // (every sub-session holds the mask and the anchors, as in sfa_session_targets)
    if (s->spread) return spread_all(s, who, [&](sfa_session *sub) { return sfa_session_targets_reach(sub, targets, n); });
    sfa_ctx *c = s->c;
    if (int rc = refuse_wide(c, who, "classes")) return rc;
    const HostModel hm(s);
    char msg[224];
    if (sfa::reach_list_error(targets, n, hm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    sfa::ReachPrepared prep;
    sfa::reach_prepare(targets, n, hm.m, &prep);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a mask in use is not replaced under a kernel)
    if (int rc = reach_build(s, prep, who)) return targets_give_up(s, rc);
    if (s->cover.on()) return cover_derive(s, who);  // (the depth is kept: the live mask of the new base mask and its anchors)
    return SFA_OK;
}

int sfa_session_reach_tables(sfa_session_t *s, uint32_t *mask, size_t n_words, int32_t *anchor, int64_t n_cols) {
    static const char *const who = "sfa_session_reach_tables";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (int rc = spread_live(s, who)) return rc;
    if (s->spread) return sfa_session_reach_tables(state_of(s), mask, n_words, anchor, n_cols);  // (shard 0 answers: every shard holds the same tables)
    sfa_ctx *c = s->c;
    if (!s->reach.on) return fail(SFA_EINVAL, "%s: the session has no reach targets (sfa_session_targets_reach)", who);
    const size_t words = sfa::target_mask_words(c->model.total_cols);
    if (mask && n_words != words) return fail(SFA_EINVAL, "%s: n_words is %zu; the mask has %zu words", who, n_words, words);
    if (anchor && n_cols != c->model.total_cols) return fail(SFA_EINVAL, "%s: n_cols is %lld; a row has %lld columns", who, (long long)n_cols, (long long)c->model.total_cols);
    HIP_TRY(hipSetDevice(c->device));
    if (mask) HIP_TRY(hipMemcpyAsync(mask, s->targets.d_mask.p, 4 * words, hipMemcpyDeviceToHost, c->stream));
    if (anchor) HIP_TRY(hipMemcpyAsync(anchor, s->reach.d_anchor.p, 4 * static_cast<size_t>(n_cols), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SFA_OK;
}

// ---- coverage caps (coverage_rules.hpp, sdtw_session_cover.hpp) ----

size_t sfa_session_coverage_bytes(const sfa_ref_t *ref, int flag) {
    int64_t entries = 0, cols = 0;
    return ref_columns(ref, flag, &entries, &cols) ? sfa::coverage_bytes(entries, cols) : 0;
}

int sfa_session_coverage_config(sfa_session_t *s, int32_t cap) {
    static const char *const who = "sfa_session_coverage_config";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (cap < 0 || cap > sfa::kCoverCapMax) return fail(SFA_EINVAL, "%s: cap must be 0 (off) .. %d, not %d", who, sfa::kCoverCapMax, cap);
    if (int rc = spread_live(s, who)) return rc;
    if (cap > 0 && !state_of(s)->targets.on) return fail(SFA_EINVAL, "%s: the session has no targets (sfa_session_targets)", who);
    if (s->spread) return spread_all(s, who, [&](sfa_session *sub) { return sfa_session_coverage_config(sub, cap); });
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a mask in use is not replaced under a kernel)
    if (cap == 0) {
        mask_cap_off(s);
        return SFA_OK;
    }
    if (int rc = cover_track_up(s, !s->gcover.on())) return rc;  // (a group cap's depth is kept: the track is the session's one)
    int rc = v.reserve_mask(c->model.total_cols);
    if (!rc) {
        HIP_TRY(hipMemsetAsync(v.d_live.p, 0, 4 * sfa::target_mask_words(c->model.total_cols), c->stream));  // (the spare word stays zero)
        v.cap = cap;
        rc = cover_derive(s, who);  // (without a group cap the depth is 0 everywhere: the live mask is the base mask)
    }
    if (rc) mask_cap_off(s);
    return rc;
}

int sfa_session_coverage_add(sfa_session_t *s, const sfa_target_t *iv, int32_t n, int64_t *open_columns) {
    static const char *const who = "sfa_session_coverage_add";
    if (!s || n < 0 || (n > 0 && !iv)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (n > sfa::kCoverIntervalsMax) return fail(SFA_EINVAL, "%s: %d intervals in one call; at most %d", who, n, sfa::kCoverIntervalsMax);
    if (int rc = spread_live(s, who)) return rc;
    sfa_session *first = state_of(s);
    if (!first->cover.on() && !first->gcover.on()) return fail(SFA_EINVAL, "%s: the session has no coverage cap (sfa_session_coverage_config)", who);
    {
        const HostModel hm(first);
        char msg[192];
        if (sfa::coverage_list_error(iv, n, hm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    }
    if (s->spread) {
        if (int rc = spread_all(s, who, [&](sfa_session *sub) { return sfa_session_coverage_add(sub, iv, n, nullptr); })) return rc;
        if (open_columns) *open_columns = sfa_session_target_columns(first);  // (shard 0's count: every shard holds the same mask)
        return SFA_OK;
    }
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    HIP_TRY(hipEventRecord(v.ev[0], st));
    if (n > 0) {
        if (int rc = v.reserve_call(static_cast<size_t>(n))) return rc;
        memcpy(v.h_iv.p, iv, sizeof(sfa_target_t) * static_cast<size_t>(n));
        HIP_TRY(hipMemcpyAsync(v.d_iv.p, v.h_iv.p, sizeof(sfa_target_t) * static_cast<size_t>(n), hipMemcpyHostToDevice, st));
        sfa::SessionCoverAddArgs a;
        a.iv = v.d_iv.as<sfa_target_t>();
        a.cov_off = v.d_cov_off.as<int64_t>();
        a.ref_len = c->model.d_ref_len.as<int32_t>();
        a.ref_st_offset = c->model.d_ref_off.as<int32_t>();
        a.depth = v.d_depth.as<uint32_t>();
        a.n = n;
        hipLaunchKernelGGL(sfa::session_cover_add_kernel, dim3(static_cast<unsigned>(n)), dim3(sfa::kCoverThreads), 0, st, a);
        KERNEL_TRY();
    }
    // whichever of the live mask and the live labels are on, from the one track, in this call
    if (v.on())
        if (int rc = cover_enqueue_mask(s)) return rc;
    if (s->gcover.on())
        if (int rc = gcover_enqueue_labels(s)) return rc;
    HIP_TRY(hipEventRecord(v.ev[1], st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    if (v.on()) cover_collect(s);
    if (s->gcover.on()) gcover_collect(s);
    HIP_TRY(hipEventElapsedTime(&v.ms, v.ev[0], v.ev[1]));
    call_profile(c, v.ms);
    if (open_columns) *open_columns = sfa_session_target_columns(s);  // (the live columns under a mask cap; without one the mask's own)
    return SFA_OK;
}

int sfa_session_coverage_depth(sfa_session_t *s, int32_t contig, uint32_t *out, int32_t n) {
    static const char *const who = "sfa_session_coverage_depth";
    if (!s || !out) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = spread_live(s, who)) return rc;
    if (s->spread) return sfa_session_coverage_depth(state_of(s), contig, out, n);  // (shard 0 answers, on the caller's thread as in for_each_shard)
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    if (!v.on() && !s->gcover.on()) return fail(SFA_EINVAL, "%s: the session has no coverage cap (sfa_session_coverage_config)", who);
    if (contig < 0 || contig >= c->model.num_ref) return fail(SFA_EINVAL, "%s: contig %d out of range (the reference has %d)", who, contig, c->model.num_ref);
    const int64_t len = v.h_cov_off[static_cast<size_t>(contig) + 1] - v.h_cov_off[static_cast<size_t>(contig)];
    if (n != len) return fail(SFA_EINVAL, "%s: contig %d has %lld entries (ref_length + 1), not %d", who, contig, static_cast<long long>(len), n);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, v.d_depth.as<uint32_t>() + v.h_cov_off[static_cast<size_t>(contig)], 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SFA_OK;
}

// ---- group caps (group_cover_rules.hpp, sdtw_session_groupcover.hpp) ----

size_t sfa_session_group_coverage_bytes(const sfa_ref_t *ref, int flag, int32_t n_groups) {
    int64_t entries = 0, cols = 0;
    if (n_groups < 1 || n_groups > sfa::kGroupMax || !ref_columns(ref, flag, &entries, &cols)) return 0;
    return 4 * static_cast<size_t>(entries) + sess::GroupCover::bytes(cols, n_groups);
}

int sfa_session_group_coverage_config(sfa_session_t *s, int32_t cap) {
    static const char *const who = "sfa_session_group_coverage_config";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (cap < 0 || cap > sfa::kGroupCapMax) return fail(SFA_EINVAL, "%s: cap must be 0 (off) .. %d, not %d", who, sfa::kGroupCapMax, cap);
    if (int rc = spread_live(s, who)) return rc;
    if (cap > 0 && !state_of(s)->groups.on()) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (s->spread) return spread_all(s, who, [&](sfa_session *sub) { return sfa_session_group_coverage_config(sub, cap); });
    sfa_ctx *c = s->c;
    sess::GroupCover &gc = s->gcover;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a table in use is not replaced under a kernel)
    if (cap == 0) {
        group_cap_off(s);
        return SFA_OK;
    }
    // (a mask cap's depth is kept: the track is the session's one.  Whatever fails from here on leaves the group cap off)
    int rc = cover_track_up(s, !s->cover.on());
    if (!rc) rc = gc.reserve(c->model.total_cols, s->groups.n_groups);
    if (!rc) rc = sess::create_events(gc.ev, 2);
    if (!rc) {
        gc.cap = cap;
        rc = gcover_derive(s, who);
    }
    if (rc) group_cap_off(s);
    return rc;
}

int sfa_session_group_coverage(sfa_session_t *s, sfa_group_cover_t *out, int32_t n) {
    static const char *const who = "sfa_session_group_coverage";
    if (!s || !out) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = spread_live(s, who)) return rc;
    if (s->spread) return sfa_session_group_coverage(state_of(s), out, n);  // (shard 0 answers: every shard holds the same tables and tracks)
    sfa_ctx *c = s->c;
    sess::GroupCover &gc = s->gcover;
    if (!gc.on()) return fail(SFA_EINVAL, "%s: the session has no group cap (sfa_session_group_coverage_config)", who);
    const int32_t entries = s->groups.n_groups + 1;
    if (n != entries) return fail(SFA_EINVAL, "%s: the session has %d entries (n_groups + 1), not %d", who, entries, n);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    sfa_group_cover_t *hr = gc.h_rec.as<sfa_group_cover_t>();
    std::fill(hr, hr + entries, sfa::group_cover_none());
    HIP_TRY(hipEventRecord(gc.ev[0], st));
    HIP_TRY(hipMemcpyAsync(gc.d_rec.p, hr, sizeof(sfa_group_cover_t) * static_cast<size_t>(entries), hipMemcpyHostToDevice, st));  // the reset in front of the launch
    const dim3 grid(sfa::group_cover_blocks(c->model.total_cols)), block(sfa::kGroupCoverThreads);
    if (s->greach.on) {  // (a reach label table: the '+' jobs' body columns only)
        auto a = group_cover_args<sfa::SessionReachLabelGroupArgs>(s);
        a.anchor = s->greach.d_anchor.as<int32_t>();
        a.rec = gc.d_rec.as<sfa_group_cover_t>();
        hipLaunchKernelGGL(sfa::session_reach_label_group_kernel, grid, block, 0, st, a);
    } else {
        auto a = group_cover_args<sfa::SessionCoverGroupArgs>(s);
        a.rec = gc.d_rec.as<sfa_group_cover_t>();
        hipLaunchKernelGGL(sfa::session_cover_group_kernel, grid, block, 0, st, a);
    }
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(gc.ev[1], st));
    HIP_TRY(hipMemcpyAsync(hr + entries, gc.d_rec.p, sizeof(sfa_group_cover_t) * static_cast<size_t>(entries), hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, gc.ev[0], gc.ev[1]));
    call_profile(c, ms);
    memcpy(out, hr + entries, sizeof(sfa_group_cover_t) * static_cast<size_t>(entries));
    return SFA_OK;
}

// ---- target groups (group_rules.hpp, sdtw_session_group.hpp) ----

int sfa_session_target_groups(sfa_session_t *s, const sfa_group_target_t *targets, int32_t n, int32_t n_groups) {
    static const char *const who = "sfa_session_target_groups";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = refuse_resweep(s, who)) return rc;
    // (every sub-session holds the table; no slot needs to be empty, so this is spread_all, not spread_config)
    if (s->spread) return spread_all(s, who, [&](sfa_session *sub) { return sfa_session_target_groups(sub, targets, n, n_groups); });
    sfa_ctx *c = s->c;
    sess::Groups &g = s->groups;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a table in use is not replaced under a kernel)
    s->open.first.clear();                     // (sfa_session_open_classes looks for the labels' first columns again)
    if (n == 0) {
        groups_off(s);
        return SFA_OK;
    }
    if (int rc = refuse_wide(c, who, "groups")) return rc;
    const HostModel hm(s);
    char msg[256];
    if (sfa::group_list_error(targets, n, n_groups, hm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    std::vector<uint16_t> label;
    sfa::group_labels(targets, n, n_groups, hm.m, &label);
    if (int rc = g.reserve(c->model.total_cols)) return rc;
    // (the live table's tables follow the new n_groups; a group cap never outlives a failure from here on)
    int rc = s->gcover.on() ? s->gcover.reserve(c->model.total_cols, n_groups) : static_cast<int>(SFA_OK);
    if (!rc) {
        g.n_groups = 0;  // (off until the new table is up)
        s->greach.free_all();  // (a plain table replaces a reach list, before the table is overwritten: no anchor outlives the table it belongs to)
        g.h_label.swap(label);
        rc = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(g.d_label.p, g.h_label.data(), 2 * g.h_label.size(), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return SFA_OK;
        }();
    }
    if (!rc) {
        g.n_groups = n_groups;
        if (s->gcover.on()) rc = gcover_derive(s, who);  // (the depth is kept: the live table of the new base table)
    }
    if (rc && s->gcover.on()) group_cap_off(s);
    return rc;
}

int32_t sfa_session_group_count(sfa_session_t *s) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_group_count: null session");
    return state_of(s)->groups.n_groups;
}

int sfa_session_group_bests(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_group_best_t *bests, sfa_group_head_t *heads) {
    static const char *const who = "sfa_session_group_bests";
    if (!s || n < 0 || (n > 0 && (!slot || !heads))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = spread_live(s, who)) return rc;
    const int32_t entries = state_of(s)->groups.n_groups + 1;
    if (entries == 1) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (s->spread)
        return spread_query(s, slot, n, who, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
            b.ghead.resize(p.local.size());
            if (bests) b.gbest.resize(p.local.size() * static_cast<size_t>(entries));
            if (int rc = sfa_session_group_bests(sub, p.local.data(), p.n(), bests ? b.gbest.data() : nullptr, b.ghead.data())) return rc;
            if (bests) sfa::spread_scatter(p, b.gbest.data(), bests, entries);
            sfa::spread_scatter(p, b.ghead.data(), heads);
            return static_cast<int>(SFA_OK);
        });
    GroupQuery q{s, bests, heads, n};
    return query_run(s, slot, n, who, q);
}

int sfa_group_decide(const sfa_group_head_t *h, int32_t min_events, float margin) { return h ? sfa::group_decide(*h, min_events, margin) : -1; }

// ---- reach groups (reach_group_rules.hpp, sdtw_session_reachgroup.hpp) ----

size_t sfa_session_group_reach_bytes(const sfa_ref_t *ref, int flag) {
    int64_t entries = 0, cols = 0;
    return ref_columns(ref, flag, &entries, &cols) ? sfa::reach_group_bytes(cols) : 0;
}

int sfa_session_target_groups_reach(sfa_session_t *s, const sfa_reach_group_target_t *targets, int32_t n, int32_t n_groups) {
    static const char *const who = "sfa_session_target_groups_reach";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = refuse_resweep(s, who)) return rc;
    if (n == 0) return sfa_session_target_groups(s, nullptr, 0, n_groups);  // (groups off, the anchors freed: one path)
    // (every sub-session holds the table and its anchors, as in sfa_session_target_groups)
    if (s->spread) return spread_all(s, who, [&](sfa_session *sub) { return sfa_session_target_groups_reach(sub, targets, n, n_groups); });
    sfa_ctx *c = s->c;
    if (int rc = refuse_wide(c, who, "groups")) return rc;
    const HostModel hm(s);
    char msg[256];
    if (sfa::reach_group_list_error(targets, n, n_groups, hm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    sfa::ReachGroupPrepared prep;
    sfa::reach_group_prepare(targets, n, hm.m, &prep);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a table in use is not replaced under a kernel)
    if (int rc = reach_group_build(s, prep, n_groups, who)) return groups_give_up(s, rc);
    if (s->gcover.on())  // (the depth is kept: the live table of the new base table and its anchors)
        if (int rc = gcover_derive(s, who)) return groups_give_up(s, rc);
    return SFA_OK;
}

int sfa_session_group_reach_tables(sfa_session_t *s, uint16_t *label, int32_t *anchor, int64_t n_cols) {
    static const char *const who = "sfa_session_group_reach_tables";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (int rc = spread_live(s, who)) return rc;
    if (s->spread) return sfa_session_group_reach_tables(state_of(s), label, anchor, n_cols);  // (shard 0 answers: every shard holds the same tables)
    sfa_ctx *c = s->c;
    if (!s->greach.on) return fail(SFA_EINVAL, "%s: the session has no reach groups (sfa_session_target_groups_reach)", who);
    if ((label || anchor) && n_cols != c->model.total_cols)
        return fail(SFA_EINVAL, "%s: n_cols is %lld; a row has %lld columns", who, (long long)n_cols, (long long)c->model.total_cols);
    HIP_TRY(hipSetDevice(c->device));
    if (label) HIP_TRY(hipMemcpyAsync(label, s->groups.d_label.p, 2 * static_cast<size_t>(n_cols), hipMemcpyDeviceToHost, c->stream));
    if (anchor) HIP_TRY(hipMemcpyAsync(anchor, s->greach.d_anchor.p, 4 * static_cast<size_t>(n_cols), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SFA_OK;
}

// ---- open and closed groups (quota_rules.hpp, sdtw_session_open.hpp) ----

int sfa_session_open_classes(sfa_session_t *s, const int32_t *slot, int32_t n, const uint32_t *open, int32_t n_words, sfa_open_class_t *out) {
    static const char *const who = "sfa_session_open_classes";
    if (!s || n < 0 || (n > 0 && (!slot || !out))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (int rc = spread_live(s, who)) return rc;
    const int32_t n_groups = state_of(s)->groups.n_groups;
    if (n_groups == 0) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (open && n_words != sfa::open_words(n_groups))
        return fail(SFA_EINVAL, "%s: the bitmap of %d groups has %d words, not %d", who, n_groups, sfa::open_words(n_groups), n_words);
    if (s->spread)
        return spread_query(s, slot, n, who, [&](sfa_session *sub, const sfa::SpreadShardPart &p, sess::Spread::Shard &b) {
            b.ocls.resize(p.local.size());
            if (int rc = sfa_session_open_classes(sub, p.local.data(), p.n(), open, n_words, b.ocls.data())) return rc;
            sfa::spread_scatter(p, b.ocls.data(), out);
            return static_cast<int>(SFA_OK);
        });
    OpenQuery q{s, open, out, n};
    return query_run(s, slot, n, who, q);
}

}  // extern "C"
