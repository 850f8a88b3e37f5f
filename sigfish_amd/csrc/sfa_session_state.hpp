// sfa_session_state.hpp -- what the two units of the alignment sessions share (private to the library): the session itself, its
// state one struct per feature that owns it (namespace sess, as namespace ctx of sfa_ctx.hpp), and the prologue every entry point
// begins with -- the slots a call names, and on a spread session the partition and the visit of the shards.
//   sfa_session.hip          creation, the sweep behind both extend entry points, raw mode, event maps, spread sessions
//   sfa_session_targets.hip  targets, groups, caps and reach lists, and the three query calls that read a slot's carried row
// The session's state, each struct with its buffers, what it keeps between calls and reserve(), the sizes:
//   sess::Rows        the carried rows, the slots' current rows, lengths, poison flags and call stamps
//   sess::Sweep       what one sweep needs: events, staging, poison flags of the call (the raw path writes them too), partial results
//   sess::Candidates  sfa_session_candidates_config: the lists behind every slot's row
//   sess::Raw         raw mode (sfa_session_raw_config, events_stream.hpp): detector states, event tables, normalised queries, the
//                     recalibration rule, the tables of a call -- samples go in, events and query stay on the device
//   sess::AutoStart   sfa_session_raw_auto_start (events_auto_stream.hpp): retained samples, the slots' targets and skips
//   sess::Keep        sfa_session_keep_events: the events of an event-mode session's slots, kept for their maps
//   sess::Maps        sfa_session_event_maps: the scratch of a call (the core is sfa_maps.hip's), where every slot's query begins
//   sess::Query       of a query call (sfa_session_classes, _group_bests, _open_classes): the entries launched, their slots, the times
//   sess::Targets     sfa_session_targets: the column mask, and of a sfa_session_classes call the partial minima, results
//   sess::Groups      sfa_session_target_groups: the label table, and of a sfa_session_group_bests call the keys, results
//   sess::Open        sfa_session_open_classes: the lowest column of every label, and of a call the partial minima, results
//   sess::Coverage    sfa_session_coverage_config: the depth tracks, the live mask, and of a sfa_session_coverage_add call the intervals
//   sess::Reach       sfa_session_targets_reach: the anchors beside a mask that was built from a reach list
//   sess::GroupReach  sfa_session_target_groups_reach: the anchors beside a label table that was built from a reach group list
//   sess::GroupCover  sfa_session_group_coverage_config: the live label table, its labels' first columns, the groups' depth records
//   sess::Spread      SFA_SESSION_SPREAD on a group context: one sub-session per shard, a call's entries dealt to them
// The host rules -- which waves a call becomes, which points of the automatic start it passes -- are session_plan.hpp's; which
// entries of a query call launch, session_query.hpp's; where a spread session's slots live and how a call is dealt to the shards,
// session_spread.hpp's.
#pragma once
#include "sfa_ctx.hpp"
#include "sdtw_session.hpp"  // (the unit that defines SFA_DEFINE_SESSION_KERNELS in front of this header holds the plain kernels)
#include "events_stream.hpp"
#include "session_query.hpp"
#include "session_spread.hpp"
#include "sdtw_session_class.hpp"
#include "sdtw_session_group.hpp"
#include "sdtw_session_open.hpp"
#include "sdtw_session_cover.hpp"
#include "sdtw_session_groupcover.hpp"
#include "sdtw_session_reach.hpp"
#include "sdtw_session_reachgroup.hpp"

// ---- the session's state, one struct per feature that owns it (as namespace ctx of sfa_ctx.hpp) ----
namespace sess {

inline int create_events(Event *ev, int n) {
    for (int i = 0; i < n; ++i)
        if (!ev[i].h && hipEventCreate(&ev[i].h) != hipSuccess) return fail(SFA_ENODEV, "hipEventCreate failed");
    return SFA_OK;
}

struct Rows {  // the carried rows and the per-slot host state
    DevBuf d_row_c, d_row_s;         // carried rows: costs, start columns
    DevBuf d_col_off;                // [n_jobs] first column of every job inside a slot's row
    std::vector<int64_t> h_col_off;
    DevBuf d_rows;                   // [n_slots] the slots' current rows
    PinBuf h_rows;
    std::vector<int64_t> len;        // events every slot has received since its last reset
    std::vector<uint8_t> poison;     // a chunk of the slot held a NaN / inf: no rows until reset
    std::vector<int32_t> stamp;      // call in which the slot was named last (duplicates inside one call)
    static int64_t slot_bytes(int64_t total_cols, bool track) { return total_cols * (track ? 8 : 4); }  // one row, updated in place: costs, start columns
    int reserve(int64_t total_cols, int32_t n_slots, size_t n_jobs, bool track) {
        const size_t plane = static_cast<size_t>(slot_bytes(total_cols, false)) * n_slots + 4 * 2 * sfa::kSessionPad, rows = sizeof(sfa_result_t) * n_slots;
        len.assign(n_slots, 0), poison.assign(n_slots, 0), stamp.assign(n_slots, 0), h_col_off.resize(n_jobs);
        if (int rc = reserve_all(d_row_c, plane, d_col_off, 8 * n_jobs, d_rows, rows, h_rows, rows)) return rc;
        return track ? d_row_s.reserve(plane) : SFA_OK;
    }
};

struct Sweep {  // of a call of the sweep
    DevBuf d_events, d_stage, d_bad, d_count, d_pbest, d_psecond, d_pend, d_pst;
    PinBuf h_stage, h_bad;
    std::vector<sfa::Launch> launches;   // the call's plan (session_plan.hpp), its argument block per launch, bytes staged
    std::vector<int32_t> call_slot;
    std::vector<sfa::SessionArgs> args;
    size_t staged = 0;
    size_t keep_at = 0;  // where the keep kernel's tables lie in the staging (0: the call keeps nothing)
    Event ev[4];  // first kernel, sweeps start / end, rows written
    // the call's poison flags: the screen writes them, or the raw path's normalisation before the sweep (same n: nothing is dropped)
    int reserve_bad(size_t n) { return reserve_all(d_bad, n, h_bad, n + 8); }
    int reserve_count() { return d_count.reserve(64); }  // (the screen's counter: once, at creation)
    int reserve(size_t stage_bytes, int64_t nq, size_t n, size_t n_part) {
        if (int rc = reserve_bad(n)) return rc;
        return reserve_all(h_stage, stage_bytes, d_stage, stage_bytes, d_events, sizeof(float) * static_cast<size_t>(std::max<int64_t>(nq, 1)), d_pbest,
                           4 * n_part, d_psecond, 4 * n_part, d_pend, 4 * n_part, d_pst, 4 * n_part);
    }
};

struct Candidates {  // sfa_session_candidates_config
    int32_t n_cand = 0;   // candidates kept behind every slot's row (0: none, the plain kernels)
    DevBuf d_cand, d_p5;  // [n_slots][4] the slots' candidates; of a call: [n][n_jobs] lists of kTop5Words words
    PinBuf h_cand;
    static size_t bytes(int32_t n_slots) { return sizeof(sfa_result_t) * 4 * static_cast<size_t>(n_slots); }
    int reserve(int32_t n_slots) { return reserve_all(d_cand, bytes(n_slots), h_cand, bytes(n_slots)); }
    int reserve_call(size_t n_part) { return n_cand > 0 ? d_p5.reserve(4 * sfa::kTop5Words * n_part) : SFA_OK; }
};

struct Raw {  // raw mode and its recalibration rule
    bool on = false;
    int32_t skip = 0, norm = 0, query = 0;  // (with the automatic start `skip` is the largest skip a slot may resolve)
    struct Slot {
        int64_t n = 0;                // samples received since the last reset
        int32_t nev = 0, status = 0;  // its final events; bits of sfa_session_raw_info_t.status
        float mean = 0.0f, sd = 0.0f;
        int32_t window = 0;           // events the mean and sd span (0: not calibrated)
        uint8_t fresh = 1;            // no chunk since the last reset: the next one initialises the detector state (ev_stream_kernel)
        double scaling[3] = {0, 0, 0};  // latched by the first chunk after a reset
    };
    std::vector<Slot> slots;
    DevBuf d_state, d_evtab, d_query;  // [n_slots] EvStreamSlot, [n_slots][skip + query] EvRecord, [n_slots][query] float
    DevBuf d_window;                   // [n_slots] i32: the window a calibrated slot's normalisation spans (EvNormArgs.window)
    int32_t recal_at[sfa::kRecalMaxPoints] = {0};  // sfa_session_raw_recalibrate: the points, their number, the flags
    int32_t recal_n = 0;
    uint32_t recal_flags = 0;
    DevBuf d_raw, d_rstage, d_rout;    // of a call: samples, entry tables, EvStreamOut per entry
    PinBuf h_rstage, h_rout;
    std::vector<float> scale;          // ... its [n][2] offset and range / digitisation, the detector's argument block,
    sfa::EvStreamArgs ea;              // where the automatic start's tables lie in the staging, the bytes staged
    size_t o_have = 0, o_aent = 0, staged = 0;
    Event ev_raw[3];                   // detector start / end, normalisation end
    DevBuf d_span_in, d_span;          // of a sfa_session_query_span call: [slot n | q_events n (| skip n)] x i32, [n][2] u64
    PinBuf h_span_in, h_span;
    int32_t ev_cap() const { return skip + query; }
    static int64_t evtab_bytes(int32_t skip_events, int32_t query_events) { return (static_cast<int64_t>(skip_events) + query_events) * static_cast<int64_t>(sizeof(sfa::EvRecord)); }
    static int64_t slot_bytes(int32_t skip_ev, int32_t query_ev) { return evtab_bytes(skip_ev, query_ev) + 4 * static_cast<int64_t>(query_ev) + static_cast<int64_t>(sizeof(sfa::EvStreamSlot)); }
    int reserve(int32_t n_slots, int32_t skip_events, int32_t query_events) {
        const size_t ns = static_cast<size_t>(n_slots);
        return reserve_all(d_state, sizeof(sfa::EvStreamSlot) * ns, d_evtab, static_cast<size_t>(evtab_bytes(skip_events, query_events)) * ns, d_query,
                           4 * static_cast<size_t>(query_events) * ns, d_window, 4 * ns);
    }
    int reserve_call(size_t stage_bytes, int64_t total, size_t n) {
        return reserve_all(h_rstage, stage_bytes, d_rstage, stage_bytes, d_raw, 2 * static_cast<size_t>(std::max<int64_t>(total, 1)), d_rout, sizeof(sfa::EvStreamOut) * n, h_rout,
                           sizeof(sfa::EvStreamOut) * n);
    }
    int reserve_span(size_t in_bytes, size_t n) { return reserve_all(h_span_in, in_bytes, d_span_in, in_bytes, d_span, 16 * n, h_span, 16 * n); }
    void reset_slot(int32_t sl) { slots[sl] = Slot{}; }
};

struct AutoStart {  // automatic query start (sfa_session_raw_auto_start)
    int32_t every = 0, max_samples = 0;      // max_samples 0: off
    struct Slot {
        sfa::EvAutoSlot h{-1, -1, 0, sfa::kAutoPending};  // what the slot's device state holds (read back by each call)
        int32_t k = 0;                                    // periodic points N_k it has passed
        bool final_taken = false;                         // its final point has been taken
    };
    std::vector<Slot> slots;
    int32_t n_pending = 0;                   // of a call: its slots with a pending point
    std::vector<sfa::AutoPoints> call;       // [n_slots] of a call: what auto_points said for entry i (a call names a slot once: n <= n_slots)
    DevBuf d_auto, d_keep, d_csum, d_aout;   // [n_slots] EvAutoSlot, [n_slots][max_samples] i16, of a call: prefix sums, EvAutoSlot per entry
    PinBuf h_aout;
    Event ev_auto[2];                        // retention + evaluation of a call: start, end
    float ms = 0.0f;                         // ... their time in the last call (sfa_session_auto_ms)
    bool on() const { return max_samples > 0; }
    static int64_t keep_bytes(int32_t max) { return 2 * static_cast<int64_t>(max); }        // retention (int16)
    static int64_t csum_bytes(int32_t max) { return 4 * (static_cast<int64_t>(max) + 1); }  // prefix sums of a slot with a pending point
    static int64_t slot_bytes(int32_t max) { return keep_bytes(max) + static_cast<int64_t>(sizeof(sfa::EvAutoSlot)) + csum_bytes(max); }
    int reserve(int32_t n_slots, int32_t max) {
        return reserve_all(d_auto, sizeof(sfa::EvAutoSlot) * static_cast<size_t>(n_slots), d_keep, static_cast<size_t>(keep_bytes(max)) * n_slots);
    }
    int reserve_call(int32_t n_pending, size_t n) {
        return reserve_all(d_csum, static_cast<size_t>(csum_bytes(max_samples)) * static_cast<size_t>(std::max(n_pending, 1)), d_aout, sizeof(sfa::EvAutoSlot) * n, h_aout,
                           sizeof(sfa::EvAutoSlot) * n);
    }
    void reset_slot(int32_t sl) { slots[sl] = Slot{}; }
};

struct Keep {  // sfa_session_keep_events (event mode)
    int32_t max_events = 0;  // 0: off
    DevBuf d_keep, d_over;   // [n_slots][max_events] float, [n_slots] u8: the slot outgrew max_events
    PinBuf h_over;
    bool on() const { return max_events > 0; }
    static int64_t slot_bytes(int32_t max) { return 4 * static_cast<int64_t>(max); }
    int reserve(int32_t n_slots, int32_t max) {
        const size_t ns = static_cast<size_t>(n_slots);
        return reserve_all(d_keep, static_cast<size_t>(slot_bytes(max)) * ns, d_over, ns, h_over, ns);
    }
};

struct Maps {  // sfa_session_event_maps
    ctx::MapScratch scratch;      // moves, row table, device output of a call: the session's own, never the context's
    std::vector<int64_t> q_off;   // [n_slots] where every slot's query begins behind the query base
    std::vector<sfa::MapRow> band;  // of a call
    int reserve(int32_t n_slots, size_t n_rows) {  // (the scratch grows slice by slice inside the core)
        q_off.resize(static_cast<size_t>(n_slots));
        band.assign(n_rows, sfa::MapRow{});
        return SFA_OK;
    }
};

// What the three query calls share (query_run, sfa_session_targets.hip).  One of it is enough: a query call runs on the context's
// stream and synchronises before it returns, so no two of them overlap on a session.
struct Query {
    std::vector<int32_t> live;            // which entries of the call are launched (session_query.hpp), in the caller's order
    DevBuf d_slot;                        // [m] i32: their slots
    PinBuf h_slot;
    Event ev[2];                          // in front of and behind the call's two launches
    int reserve(size_t m) {
        if (int rc = reserve_all(d_slot, 4 * m, h_slot, 4 * m)) return rc;
        return create_events(ev, 2);
    }
};

struct Targets {  // sfa_session_targets, sfa_session_classes
    bool on = false;
    int64_t on_cols = 0;                  // on-target columns of a slot's row
    int32_t first_on = -1, first_off = -1;  // lowest column of either class (-1: the class is empty)
    std::vector<uint32_t> h_mask;         // of the last sfa_session_targets call (the upload is synchronous: pageable is fine)
    DevBuf d_mask;                        // target_mask_words(total_cols) words
    DevBuf d_part, d_cls;                 // of a call: [n][parts] ClassPartial, [n] sfa_class_t
    PinBuf h_cls;
    static size_t mask_bytes(int64_t total_cols) { return 4 * sfa::target_mask_words(total_cols); }  // one bit per column, and a word
    int reserve(int64_t total_cols) { return d_mask.reserve(mask_bytes(total_cols)); }
    int reserve_call(size_t n, size_t parts) { return reserve_all(d_part, sizeof(sfa::ClassPartial) * n * parts, d_cls, sizeof(sfa_class_t) * n, h_cls, sizeof(sfa_class_t) * n); }
};

struct Groups {  // sfa_session_target_groups, sfa_session_group_bests
    int32_t n_groups = 0;                 // 0: off
    std::vector<uint16_t> h_label;        // of the last sfa_session_target_groups call (the upload is synchronous: pageable is fine)
    DevBuf d_label;                       // group_label_words(total_cols) words of four labels
    DevBuf d_key, d_best, d_head;         // of a call: [n][n_groups + 1] u64, [n][n_groups + 1] sfa_group_best_t, [n] sfa_group_head_t
    PinBuf h_best, h_head;
    bool on() const { return n_groups > 0; }
    int reserve(int64_t total_cols) { return d_label.reserve(8 * sfa::group_label_words(total_cols)); }
    int reserve_call(size_t n, size_t entries, bool bests) {
        const size_t nb = bests ? sizeof(sfa_group_best_t) * n * entries : 0;
        if (nb)
            if (int rc = reserve_all(d_best, nb, h_best, nb)) return rc;
        return reserve_all(d_key, 8 * n * entries, d_head, sizeof(sfa_group_head_t) * n, h_head, sizeof(sfa_group_head_t) * n);
    }
};

struct Open {  // sfa_session_open_classes (the label table is sess::Groups')
    std::vector<int32_t> first;           // lowest column of every label, [n_groups + 1]; empty: not looked for since the table was set
    DevBuf d_part, d_out;                 // of a call: [n][parts] ClassPartial, [n] sfa_open_class_t
    PinBuf h_out;
    int reserve(size_t n, size_t parts) { return reserve_all(d_part, sizeof(sfa::ClassPartial) * n * parts, d_out, sizeof(sfa_open_class_t) * n, h_out, sizeof(sfa_open_class_t) * n); }
};

struct Coverage {  // sfa_session_coverage_config, sfa_session_coverage_add (coverage_rules.hpp)
    int32_t cap = 0;                      // 0: off
    int64_t live_cols = 0;                // live on-target columns of a slot's row
    int32_t first_on = -1, first_off = -1;  // lowest column of either class under the live mask (-1: the class is empty)
    std::vector<int64_t> h_cov_off;       // [num_ref + 1] where every contig's track begins
    DevBuf d_depth, d_live, d_cov_off;    // the tracks, the live mask (target_mask_words words), the offsets
    DevBuf d_stats, d_iv;                 // the mask launch's CoverStats; of a call: [n] sfa_target_t
    PinBuf h_stats, h_iv;                 // [0] the record's initial value, [1] what the launch left
    Event ev[2];
    float ms = 0.0f;                      // device time of the last add + mask
    bool on() const { return cap > 0; }
    // The tracks (d_depth, d_cov_off, h_cov_off, the intervals of a call, the events) are the session's ONE depth track: the mask's
    // cap here and the group cap of sess::GroupCover share them.  Whichever is configured first reserves them; they go when both are off.
    bool has_track() const { return !h_cov_off.empty(); }
    int reserve_track(int64_t entries, int32_t num_ref) { return reserve_all(d_depth, 4 * static_cast<size_t>(entries), d_cov_off, 8 * (static_cast<size_t>(num_ref) + 1)); }
    int reserve_mask(int64_t total_cols) { return reserve_all(d_live, 4 * sfa::target_mask_words(total_cols), d_stats, sizeof(sfa::CoverStats), h_stats, 2 * sizeof(sfa::CoverStats)); }
    int reserve_call(size_t n) { return reserve_all(d_iv, sizeof(sfa_target_t) * n, h_iv, sizeof(sfa_target_t) * n); }
    void free_mask() {  // the mask's cap and what only it uses
        cap = 0, live_cols = 0, first_on = first_off = -1;
        d_live = DevBuf{}, d_stats = DevBuf{};
        h_stats = PinBuf{};
    }
    void free_track() {
        std::vector<int64_t>().swap(h_cov_off);
        d_depth = DevBuf{}, d_cov_off = DevBuf{}, d_iv = DevBuf{};
        h_iv = PinBuf{};
    }
};

struct Reach {  // sfa_session_targets_reach (reach_rules.hpp): the mask is sess::Targets', the anchors lie beside it
    bool on = false;
    DevBuf d_anchor;                      // [total_cols] i32: the anchor's entry of its contig's depth track
    DevBuf d_runs, d_run_off, d_stats;    // of a call: the prepared runs, freed when the build is through; the build launch's CoverStats
    PinBuf h_stats;                       // [0] the record's initial value, [1] what the launch left
    int reserve(int64_t total_cols, size_t n_runs, int32_t n_jobs) {
        return reserve_all(d_anchor, sfa::reach_bytes(total_cols), d_runs, sizeof(sfa::ReachRun) * (n_runs + 1), d_run_off, 4 * (static_cast<size_t>(n_jobs) + 1), d_stats,
                           sizeof(sfa::CoverStats), h_stats, 2 * sizeof(sfa::CoverStats));
    }
    void free_all() {
        on = false;
        d_anchor = DevBuf{}, d_runs = DevBuf{}, d_run_off = DevBuf{}, d_stats = DevBuf{};
        h_stats = PinBuf{};
    }
};

struct GroupReach {  // sfa_session_target_groups_reach (reach_group_rules.hpp): the label table is sess::Groups', its anchors lie beside it
    bool on = false;
    DevBuf d_anchor;                      // [total_cols] i32: the anchor's entry of its contig's depth track
    DevBuf d_runs, d_run_off, d_first;    // of a call: the prepared runs, the lowest column of every label; freed when the build is through
    PinBuf h_first;                       // [2][n_groups + 1]: the table's initial value, what the launch left
    int reserve(int64_t total_cols, size_t n_runs, int32_t n_jobs, int32_t n_groups) {
        const size_t e = static_cast<size_t>(n_groups) + 1;
        return reserve_all(d_anchor, 4 * static_cast<size_t>(total_cols), d_runs, sizeof(sfa::ReachGroupRun) * (n_runs + 1), d_run_off, 4 * (static_cast<size_t>(n_jobs) + 1), d_first,
                           4 * e, h_first, 2 * 4 * e);
    }
    void free_call() {
        d_runs = DevBuf{}, d_run_off = DevBuf{}, d_first = DevBuf{};
        h_first = PinBuf{};
    }
    void free_all() {
        on = false;
        d_anchor = DevBuf{};
        free_call();
    }
};

struct GroupCover {  // sfa_session_group_coverage_config, sfa_session_group_coverage (group_cover_rules.hpp; the tracks are sess::Coverage's)
    int32_t cap = 0;                      // 0: off
    std::vector<int32_t> first;           // lowest column of every LIVE label, [n_groups + 1], -1: none (what open_first_cols reads)
    DevBuf d_live;                        // the live label table: group_label_words(total_cols) words of four labels
    DevBuf d_first, d_rec;                // [n_groups + 1] i32; [n_groups + 1] sfa_group_cover_t
    PinBuf h_first, h_rec;                // [2][n_groups + 1]: the tables' initial values, what the launch left
    Event ev[2];
    bool on() const { return cap > 0; }
    // bytes beside the tracks (sfa_session_group_coverage_bytes adds them): what reserve() asks for, through the one function
    static size_t bytes(int64_t total_cols, int32_t n_groups) { return sfa::group_cover_bytes(total_cols, n_groups); }
    int reserve(int64_t total_cols, int32_t n_groups) {
        const size_t e = static_cast<size_t>(n_groups) + 1;
        return reserve_all(d_live, 8 * sfa::group_label_words(total_cols), d_first, 4 * e, d_rec, sizeof(sfa_group_cover_t) * e, h_first, 2 * 4 * e, h_rec, 2 * sizeof(sfa_group_cover_t) * e);
    }
    void free_all() {
        cap = 0;
        std::vector<int32_t>().swap(first);
        d_live = DevBuf{}, d_first = DevBuf{}, d_rec = DevBuf{};
        h_first = PinBuf{}, h_rec = PinBuf{};
    }
};

// SFA_SESSION_SPREAD on a group context: the session is one ordinary session per shard that holds slots (global slot i: local
// slot i / G of subs[i % G]); every entry point deals its entries to them (session_spread.hpp), runs the shards side by side
// (for_each_shard) and puts the answers back in the caller's order.  What a call packs or collects per shard lies here and is
// reused from call to call: a tick allocates nothing once the buffers have grown to its size.
struct Spread {
    std::vector<sfa_session *> subs;  // [G]; nullptr: a trailing shard of a session with fewer slots than shards
    sfa::SpreadPart part;             // of a call
    struct Shard {                    // of a call, per shard: the payload packed, per-entry arguments gathered, answers
        std::vector<float> events;
        std::vector<int16_t> raw;
        std::vector<double> scaling;
        std::vector<uint8_t> end;
        std::vector<sfa_result_t> rows;
        std::vector<sfa_session_raw_info_t> info;
        std::vector<sfa_session_auto_t> autos;
        std::vector<int64_t> len;
        std::vector<uint64_t> span;
        std::vector<sfa_class_t> cls;
        std::vector<sfa_group_best_t> gbest;
        std::vector<sfa_group_head_t> ghead;
        std::vector<sfa_open_class_t> ocls;
        int32_t on_host = 0;
    };
    std::vector<Shard> shard;  // [G]
    bool broken = false;       // a configuration call went through on some shards and failed on another: only sfa_session_destroy is left
};

}  // namespace sess

// `delete` frees every buffer and event of the session, in whatever order the members stand.  That relies on two things only:
// sfa_session_destroy has synchronised the context's stream (nothing of the session is in flight), and the stream itself is the
// context's, which sfa_destroy frees after its sessions (sfa::destroy_sessions).
struct sfa_session {
    sfa_ctx *c = nullptr;
    int32_t n_slots = 0;
    bool track = true;     // start columns are carried (no SFA_SESSION_NO_START)
    bool resweep = false;  // SFA_SESSION_RESWEEP: raw mode only; a slot is swept when its window changes, over the window's events
    int32_t call_no = 0;
    sess::Rows rows;
    sess::Sweep sweep;
    sess::Candidates cand;
    sess::Raw raw;
    sess::AutoStart autos;
    sess::Keep keep;
    sess::Maps maps;
    sess::Query query;
    sess::Targets targets;
    sess::Groups groups;
    sess::Open open;
    sess::Coverage cover;
    sess::GroupCover gcover;
    sess::Reach reach;
    sess::GroupReach greach;
    std::unique_ptr<sess::Spread> spread;  // SFA_SESSION_SPREAD on a group context: `c` is the group, everything above is unused
    int32_t name_first = 0, name_step = 1;  // a sub-session of a spread session: local slot l is the caller's slot l * step + first (messages)
};

// ---- the prologue of the entry points (both units) ----
namespace {

int check_slots(const sfa_session *s, const int32_t *slot, int32_t n, const char *who) {
    for (int32_t i = 0; i < n; ++i)
        if (slot[i] < 0 || slot[i] >= s->n_slots) return fail(SFA_EINVAL, "%s: slot %d out of range (the session has %d)", who, slot[i], s->n_slots);
    return SFA_OK;
}

// a new extend call: its number is what claim_slot stamps the slots it names with
void begin_call(sfa_session *s) {
    if (++s->call_no == INT32_MAX) {
        std::fill(s->rows.stamp.begin(), s->rows.stamp.end(), 0);
        s->call_no = 1;
    }
}

// slot sl is named by the call: in range, and once only
int claim_slot(sfa_session *s, int32_t sl, const char *who) {
    if (int rc = check_slots(s, &sl, 1, who)) return rc;
    if (s->rows.stamp[sl] == s->call_no) return fail(SFA_EINVAL, "%s: slot %d is named twice in one call", who, sl);
    s->rows.stamp[sl] = s->call_no;
    return SFA_OK;
}

// the profile of a session call that is `ms` of device time and nothing else (0: a call that launched nothing)
void call_profile(sfa_ctx *c, float ms) {
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    pr.class_ms = pr.total_ms = ms;
    c->prof = pr;
}

// ---- spread sessions: the prologue of each entry point (the rules are session_spread.hpp's) ----

// (a plain session is never broken)
int spread_live(const sfa_session *s, const char *who) {
    if (s->spread && s->spread->broken)
        return fail(SFA_EINVAL, "%s: a configuration call of this spread session failed on one shard after others had taken it; the session takes nothing but "
                                "sfa_session_destroy",
                    who);
    return SFA_OK;
}

// the call's entries by shard (left in spread->part), after the refusals a session makes by itself -- for the whole call, before
// any shard hears of it
int spread_deal(sfa_session *s, const int32_t *slot, int32_t n, bool once, const char *who) {
    const sfa::SpreadRefusal bad = sfa::spread_partition(slot, n, s->n_slots, static_cast<int32_t>(s->c->shards.size()), once, &s->spread->part);
    if (bad.why == sfa::kSpreadRange) return fail(SFA_EINVAL, "%s: slot %d out of range (the session has %d)", who, bad.slot, s->n_slots);
    if (bad.why == sfa::kSpreadTwice) return fail(SFA_EINVAL, "%s: slot %d is named twice in one call", who, bad.slot);
    return SFA_OK;
}

// fn(the shard's sub-session, its part of the call, its buffers) on every shard that has entries, side by side
template <typename F>
int spread_run(sfa_session *s, F fn) {
    sess::Spread &sp = *s->spread;
    return sfa::for_each_shard(s->c, [&](size_t r) { return sp.part.shard[r].n() == 0 ? static_cast<int>(SFA_OK) : fn(sp.subs[r], sp.part.shard[r], sp.shard[r]); });
}
// the same in turn on the caller's thread, for calls that are host arithmetic
template <typename F>
int spread_visit(sfa_session *s, F fn) {
    sess::Spread &sp = *s->spread;
    for (size_t r = 0; r < sp.subs.size(); ++r)
        if (sp.part.shard[r].n() > 0)
            if (int rc = fn(sp.subs[r], sp.part.shard[r], sp.shard[r])) return rc;
    return SFA_OK;
}

// A shard a call has nothing for does what a session call does in front of its work (a batch submitted and never waited for: its
// error is this call's) and leaves a profile that adds nothing: sfa_get_profile on the group is the slowest shard's times and the
// summed counts of THIS call
int spread_idle(sfa_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    call_profile(c, 0.0f);
    return SFA_OK;
}

// A configuration call goes to every sub-session, side by side.  What it is refused for is the same on every shard -- the
// arguments, the session's kind.  A shard that fails for a reason of its own (memory) after others have taken the call leaves the
// session in two minds: it is broken
template <typename F>
int spread_all(sfa_session *s, const char *who, F fn) {
    if (int rc = spread_live(s, who)) return rc;
    sess::Spread &sp = *s->spread;
    std::vector<int> rcs(sp.subs.size(), 0);
    const int rc = sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = fn(sp.subs[r])) : static_cast<int>(SFA_OK); });
    size_t have = 0, failed = 0;
    for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
    if (failed != 0 && failed != have) sp.broken = true;
    return rc;
}

}  // namespace
