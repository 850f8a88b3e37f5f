// sfa_session.hip -- alignment sessions of the C-ABI (include/sigfish_amd.h): a slot's subsequence DTW extended chunk by chunk
// (sdtw_session.hpp).  A session belongs to its context, runs on the context's stream and is freed with it at the latest.  Its
// state is one struct per feature (namespace sess), each with its buffers, what it keeps between calls and reserve(), the sizes:
//   sess::Rows        the carried rows, the slots' current rows, lengths, poison flags and call stamps
//   sess::Sweep       what one sweep needs: events, staging, poison flags of the call (the raw path writes them too), partial results
//   sess::Candidates  sfa_session_candidates_config: the lists behind every slot's row
//   sess::Raw         raw mode (sfa_session_raw_config, events_stream.hpp): detector states, event tables, normalised queries, the
//                     recalibration rule, the tables of a call -- samples go in, events and query stay on the device
//   sess::AutoStart   sfa_session_raw_auto_start (events_auto_stream.hpp): retained samples, the slots' targets and skips
//   sess::Keep        sfa_session_keep_events: the events of an event-mode session's slots, kept for their maps
//   sess::Maps        sfa_session_event_maps: the scratch of a call (the core is sfa_maps.hip's), where every slot's query begins
//   sess::Targets     sfa_session_targets: the column mask, and of a sfa_session_classes call the slot list, partial minima, results
//   sess::Groups      sfa_session_target_groups: the label table, and of a sfa_session_group_bests call the slot list, keys, results
//   sess::Open        sfa_session_open_classes: the lowest column of every label, and of a call the slot list, partial minima, results
//   sess::Coverage    sfa_session_coverage_config: the depth tracks, the live mask, and of a sfa_session_coverage_add call the intervals
//   sess::GroupCover  sfa_session_group_coverage_config: the live label table, its labels' first columns, the groups' depth records
//   sess::GroupReach  sfa_session_target_groups_reach: the anchors beside a label table that was built from a reach group list
//   sess::Spread      SFA_SESSION_SPREAD on a group context: one sub-session per shard, a call's entries dealt to them
// The host rules -- which waves a call becomes, which points of the automatic start it passes -- are session_plan.hpp's; where a
// spread session's slots live and how a call is dealt to the shards, session_spread.hpp's.
#include "sfa_ctx.hpp"
#define SFA_DEFINE_SESSION_KERNELS  // (this unit holds the plain kernel of sdtw_session.hpp)
#include "sdtw_session.hpp"
#include "events_stream.hpp"
#include "events_auto_stream.hpp"
#include "session_spread.hpp"
#include "sdtw_session_class.hpp"
#include "sdtw_session_group.hpp"
#include "sdtw_session_open.hpp"
#include "sdtw_session_cover.hpp"
#include "sdtw_session_groupcover.hpp"
#include "sdtw_session_reach.hpp"
#include "sdtw_session_reachgroup.hpp"

namespace sfa {
// defined in sfa_align.hip, the unit that holds the plain kernels of sdtw_kernels.hpp
__global__ void sdtw_screen_kernel(const float *queries, const int64_t *q_off, const int n, uint8_t *bad, unsigned *count);
}  // namespace sfa

// ---- the session's state, one struct per feature that owns it (as namespace ctx of sfa_ctx.hpp) ----
namespace sess {

int create_events(Event *ev, int n) {
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

struct Targets {  // sfa_session_targets, sfa_session_classes
    bool on = false;
    int64_t on_cols = 0;                  // on-target columns of a slot's row
    int32_t first_on = -1, first_off = -1;  // lowest column of either class (-1: the class is empty)
    std::vector<uint32_t> h_mask;         // of the last sfa_session_targets call (the upload is synchronous: pageable is fine)
    DevBuf d_mask;                        // target_mask_words(total_cols) words
    DevBuf d_slot, d_part, d_cls;         // of a call: [n] i32, [n][parts] ClassPartial, [n] sfa_class_t
    PinBuf h_slot, h_cls;
    std::vector<int32_t> live;            // ... which entries of the call were launched
    Event ev[2];
    static size_t mask_bytes(int64_t total_cols) { return 4 * sfa::target_mask_words(total_cols); }  // one bit per column, and a word
    int reserve(int64_t total_cols) { return d_mask.reserve(mask_bytes(total_cols)); }
    int reserve_call(size_t n, size_t parts) {
        return reserve_all(d_slot, 4 * n, h_slot, 4 * n, d_part, sizeof(sfa::ClassPartial) * n * parts, d_cls, sizeof(sfa_class_t) * n, h_cls, sizeof(sfa_class_t) * n);
    }
};

struct Groups {  // sfa_session_target_groups, sfa_session_group_bests
    int32_t n_groups = 0;                 // 0: off
    std::vector<uint16_t> h_label;        // of the last sfa_session_target_groups call (the upload is synchronous: pageable is fine)
    DevBuf d_label;                       // group_label_words(total_cols) words of four labels
    DevBuf d_slot, d_key, d_best, d_head;  // of a call: [n] i32, [n][n_groups + 1] u64, [n][n_groups + 1] sfa_group_best_t, [n] sfa_group_head_t
    PinBuf h_slot, h_best, h_head;
    std::vector<int32_t> live;            // ... which entries of the call were launched
    Event ev[2];
    bool on() const { return n_groups > 0; }
    int reserve(int64_t total_cols) { return d_label.reserve(8 * sfa::group_label_words(total_cols)); }
    int reserve_call(size_t n, size_t entries, bool bests) {
        const size_t nb = bests ? sizeof(sfa_group_best_t) * n * entries : 0;
        if (nb)
            if (int rc = reserve_all(d_best, nb, h_best, nb)) return rc;
        return reserve_all(d_slot, 4 * n, h_slot, 4 * n, d_key, 8 * n * entries, d_head, sizeof(sfa_group_head_t) * n, h_head, sizeof(sfa_group_head_t) * n);
    }
};

struct Open {  // sfa_session_open_classes (the label table is sess::Groups')
    std::vector<int32_t> first;           // lowest column of every label, [n_groups + 1]; empty: not looked for since the table was set
    DevBuf d_slot, d_part, d_out;         // of a call: [n] i32, [n][parts] ClassPartial, [n] sfa_open_class_t
    PinBuf h_slot, h_out;
    std::vector<int32_t> live;            // ... which entries of the call were launched
    Event ev[2];
    int reserve(size_t n, size_t parts) {
        return reserve_all(d_slot, 4 * n, h_slot, 4 * n, d_part, sizeof(sfa::ClassPartial) * n * parts, d_out, sizeof(sfa_open_class_t) * n, h_out, sizeof(sfa_open_class_t) * n);
    }
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

// (a slot's next chunk is a first chunk: nothing of its carried row is read)
void reset_slot(sfa_session *s, int32_t sl) {
    s->rows.len[sl] = 0;
    s->rows.poison[sl] = 0;
    if (s->raw.on) s->raw.reset_slot(sl);
    if (s->autos.on()) s->autos.reset_slot(sl);
}

// The live mask from the base mask and the depth tracks (session_cover_mask_kernel; on a reach session session_reach_live_kernel,
// which reads the depth at the column's anchor), on the context's stream; the caller has set the device and synchronises.  The
// launch in front resets the record the kernel's atomics merge into.
int cover_enqueue_mask(sfa_session *s) {
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    sfa::CoverStats *hs = v.h_stats.as<sfa::CoverStats>();
    hs[0] = sfa::CoverStats{0ull, sfa::kNoColumn, sfa::kNoColumn};
    HIP_TRY(hipMemcpyAsync(v.d_stats.p, hs, sizeof(sfa::CoverStats), hipMemcpyHostToDevice, c->stream));
    if (s->reach.on) {
        sfa::SessionReachLiveArgs a;
        a.base = s->targets.d_mask.as<uint32_t>();
        a.anchor = s->reach.d_anchor.as<int32_t>();
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
        hipLaunchKernelGGL(sfa::session_reach_live_kernel, dim3(sfa::cover_mask_blocks(c->model.total_cols)), dim3(sfa::kCoverThreads), 0, c->stream, a);
        KERNEL_TRY();
        HIP_TRY(hipMemcpyAsync(hs + 1, v.d_stats.p, sizeof(sfa::CoverStats), hipMemcpyDeviceToHost, c->stream));
        return SFA_OK;
    }
    sfa::SessionCoverMaskArgs a;
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
    hipLaunchKernelGGL(sfa::session_cover_mask_kernel, dim3(sfa::cover_mask_blocks(c->model.total_cols)), dim3(sfa::kCoverThreads), 0, c->stream, a);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(hs + 1, v.d_stats.p, sizeof(sfa::CoverStats), hipMemcpyDeviceToHost, c->stream));
    return SFA_OK;
}
// ... and what it left, once the stream is through
void cover_collect(sfa_session *s) {
    sess::Coverage &v = s->cover;
    const sfa::CoverStats &st = v.h_stats.as<sfa::CoverStats>()[1];
    v.live_cols = static_cast<int64_t>(st.live);
    v.first_on = st.first_on == sfa::kNoColumn ? -1 : st.first_on;
    v.first_off = st.first_off == sfa::kNoColumn ? -1 : st.first_off;
}
int cover_derive(sfa_session *s, const char *who) {
    if (int rc = cover_enqueue_mask(s)) return rc;
    if (hipStreamSynchronize(s->c->stream) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    cover_collect(s);
    return SFA_OK;
}

// The mask's cap goes, or the group cap; the one depth track goes with the last of them
void cover_drop_mask(sfa_session *s) {
    s->cover.free_mask();
    if (!s->gcover.on()) s->cover.free_track();
}
void gcover_drop(sfa_session *s) {
    s->gcover.free_all();
    if (!s->cover.on()) s->cover.free_track();
}

// The live label table from the base table and the depth tracks (session_cover_label_kernel; on a reach label table
// session_reach_label_live_kernel), on the context's stream; the
// caller has set the device and synchronises.  The upload in front resets the table of firsts the kernel's atomics merge into.
int gcover_enqueue_labels(sfa_session *s) {
    sfa_ctx *c = s->c;
    sess::GroupCover &gc = s->gcover;
    const size_t entries = static_cast<size_t>(s->groups.n_groups) + 1;
    int32_t *hf = gc.h_first.as<int32_t>();
    std::fill(hf, hf + entries, sfa::kNoColumn);
    HIP_TRY(hipMemcpyAsync(gc.d_first.p, hf, 4 * entries, hipMemcpyHostToDevice, c->stream));
    if (s->greach.on) {  // (a reach label table: the depth is read at the column's anchor)
        sfa::SessionReachLabelLiveArgs a;
        a.base = s->groups.d_label.as<uint64_t>();
        a.anchor = s->greach.d_anchor.as<int32_t>();
        a.live = gc.d_live.as<uint16_t>();
        a.depth = s->cover.d_depth.as<uint32_t>();
        a.cov_off = s->cover.d_cov_off.as<int64_t>();
        a.col_off = s->rows.d_col_off.as<int64_t>();
        a.ref = c->model.tables();
        a.first = gc.d_first.as<int32_t>();
        a.total_cols = c->model.total_cols;
        a.n_jobs = c->model.n_jobs;
        a.n_groups = s->groups.n_groups;
        a.cap = static_cast<uint32_t>(gc.cap);
        hipLaunchKernelGGL(sfa::session_reach_label_live_kernel, dim3(sfa::group_cover_blocks(c->model.total_cols)), dim3(sfa::kGroupCoverThreads), 0, c->stream, a);
        KERNEL_TRY();
        HIP_TRY(hipMemcpyAsync(hf + entries, gc.d_first.p, 4 * entries, hipMemcpyDeviceToHost, c->stream));
        return SFA_OK;
    }
    sfa::SessionCoverLabelArgs a;
    a.base = s->groups.d_label.as<uint64_t>();
    a.live = gc.d_live.as<uint16_t>();
    a.depth = s->cover.d_depth.as<uint32_t>();
    a.cov_off = s->cover.d_cov_off.as<int64_t>();
    a.col_off = s->rows.d_col_off.as<int64_t>();
    a.ref = c->model.tables();
    a.first = gc.d_first.as<int32_t>();
    a.total_cols = c->model.total_cols;
    a.n_jobs = c->model.n_jobs;
    a.n_groups = s->groups.n_groups;
    a.cap = static_cast<uint32_t>(gc.cap);
    hipLaunchKernelGGL(sfa::session_cover_label_kernel, dim3(sfa::group_cover_blocks(c->model.total_cols)), dim3(sfa::kGroupCoverThreads), 0, c->stream, a);
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
// are session_spread.hpp's; here the prologue of each entry point: partition, the sub-calls side by side on the context's shard
// threads (for_each_shard: shard 0 on the caller's), the answers back in the caller's order.  Calls that touch no device
// (reset, lengths, the automatic start's records) visit the shards in turn on the caller's thread ----

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

int spread_live(const sfa_session *s, const char *who) {
    if (s->spread->broken)
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

// A shard an extend call has nothing for does what a session call does in front of its work (a batch submitted and never waited
// for: its error is this call's) and leaves a profile that adds nothing: sfa_get_profile on the group is the slowest shard's
// times and the summed counts of THIS call
int spread_idle(sfa_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    c->prof = pr;
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

int spread_classes(sfa_session *s, const int32_t *slot, int32_t n, sfa_class_t *out) {
    static const char *const who = "sfa_session_classes";
    if (int rc = spread_live(s, who)) return rc;
    // (sub-session 0 exists: spread_create refuses n_slots <= 0, and shard 0 holds slot 0; every sub-session holds the same mask)
    if (!s->spread->subs[0]->targets.on) return fail(SFA_EINVAL, "%s: the session has no targets (sfa_session_targets)", who);
    if (int rc = spread_deal(s, slot, n, true, who)) return rc;
    return sfa::for_each_shard(s->c, [&](size_t r) {
        const sfa::SpreadShardPart &p = s->spread->part.shard[r];
        sess::Spread::Shard &b = s->spread->shard[r];
        if (p.n() == 0) return spread_idle(s->c->shards[r]);  // (the group's profile is this call's on every shard)
        b.cls.resize(p.local.size());
        if (int rc = sfa_session_classes(s->spread->subs[r], p.local.data(), p.n(), b.cls.data())) return rc;
        sfa::spread_scatter(p, b.cls.data(), out);
        return static_cast<int>(SFA_OK);
    });
}

int spread_group_bests(sfa_session *s, const int32_t *slot, int32_t n, sfa_group_best_t *bests, sfa_group_head_t *heads) {
    static const char *const who = "sfa_session_group_bests";
    if (int rc = spread_live(s, who)) return rc;
    // (sub-session 0 exists and every sub-session holds the same label table, as in spread_classes)
    const int32_t entries = s->spread->subs[0]->groups.n_groups + 1;
    if (entries == 1) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (int rc = spread_deal(s, slot, n, true, who)) return rc;
    return sfa::for_each_shard(s->c, [&](size_t r) {
        const sfa::SpreadShardPart &p = s->spread->part.shard[r];
        sess::Spread::Shard &b = s->spread->shard[r];
        if (p.n() == 0) return spread_idle(s->c->shards[r]);  // (the group's profile is this call's on every shard)
        b.ghead.resize(p.local.size());
        if (bests) b.gbest.resize(p.local.size() * static_cast<size_t>(entries));
        if (int rc = sfa_session_group_bests(s->spread->subs[r], p.local.data(), p.n(), bests ? b.gbest.data() : nullptr, b.ghead.data())) return rc;
        if (bests) sfa::spread_scatter(p, b.gbest.data(), bests, entries);
        sfa::spread_scatter(p, b.ghead.data(), heads);
        return static_cast<int>(SFA_OK);
    });
}

int spread_open_classes(sfa_session *s, const int32_t *slot, int32_t n, const uint32_t *open, int32_t n_words, sfa_open_class_t *out) {
    static const char *const who = "sfa_session_open_classes";
    if (int rc = spread_live(s, who)) return rc;
    // (sub-session 0 exists and every sub-session holds the same label table, as in spread_classes)
    const int32_t n_groups = s->spread->subs[0]->groups.n_groups;
    if (n_groups == 0) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (open && n_words != sfa::open_words(n_groups))
        return fail(SFA_EINVAL, "%s: the bitmap of %d groups has %d words, not %d", who, n_groups, sfa::open_words(n_groups), n_words);
    if (int rc = spread_deal(s, slot, n, true, who)) return rc;
    return sfa::for_each_shard(s->c, [&](size_t r) {
        const sfa::SpreadShardPart &p = s->spread->part.shard[r];
        sess::Spread::Shard &b = s->spread->shard[r];
        if (p.n() == 0) return spread_idle(s->c->shards[r]);  // (the group's profile is this call's on every shard)
        b.ocls.resize(p.local.size());
        if (int rc = sfa_session_open_classes(s->spread->subs[r], p.local.data(), p.n(), open, n_words, b.ocls.data())) return rc;
        sfa::spread_scatter(p, b.ocls.data(), out);
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

// A configuration call goes to every sub-session.  What it is refused for is the same on every shard -- the arguments, the
// session's kind -- but for a slot in use, which is looked for on all of them first.  A shard that fails for a reason of its own
// (memory) after others have taken the call leaves the session in two minds: it is broken
template <typename F>
int spread_config(sfa_session *s, const char *who, F fn) {
    if (int rc = spread_live(s, who)) return rc;
    sess::Spread &sp = *s->spread;
    for (const sfa_session *sub : sp.subs)
        if (sub)
            if (const int32_t sl = first_busy_slot(sub); sl >= 0)
                return fail(SFA_EINVAL, "%s: slot %d is not empty; a session is configured only while every slot is (sfa_session_reset)", who, slot_name(sub, sl));
    std::vector<int> rcs(sp.subs.size(), 0);
    const int rc = sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = fn(sp.subs[r])) : static_cast<int>(SFA_OK); });
    size_t have = 0, failed = 0;
    for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
    if (failed != 0 && failed != have) sp.broken = true;
    return rc;
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

namespace {
// a configuration call of a spread session: to every sub-session, as sfa_session_targets goes
template <class F>
int cover_spread_all(sfa_session *s, const char *who, F call) {
    if (int rc = spread_live(s, who)) return rc;
    sess::Spread &sp = *s->spread;
    std::vector<int> rcs(sp.subs.size(), 0);
    const int rc = sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = call(sp.subs[r])) : static_cast<int>(SFA_OK); });
    size_t have = 0, failed = 0;
    for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
    if (failed != 0 && failed != have) sp.broken = true;
    return rc;
}

// the reference model as the coverage rules read it (host tables; jobs are contig-major, '+' before '-': sfa_context.hip)
struct CoverModel {
    std::vector<int32_t> job_contig, ref_len;
    std::vector<int8_t> job_strand;
    sfa::TargetModel m;
    CoverModel(const sfa_session *s) {
        const sfa_ctx *c = s->c;
        const int32_t nj = c->model.n_jobs, strands = nj / c->model.num_ref;
        job_contig.resize(nj), job_strand.resize(nj), ref_len.resize(c->model.num_ref);
        for (int32_t j = 0; j < nj; ++j) job_contig[j] = j / strands, job_strand[j] = (j % strands) ? '-' : '+';
        for (int32_t r = 0; r < c->model.num_ref; ++r) ref_len[r] = c->model.h_job_len[static_cast<size_t>(r) * strands];
        m = sfa::TargetModel{c->model.num_ref, nj, job_contig.data(), job_strand.data(), c->model.h_job_len.data(), s->rows.h_col_off.data(), ref_len.data(),
                             c->model.h_ref_off.data(), c->model.total_cols};
    }
};

// The session's one depth track, for whichever cap is configured: reserved and its offsets uploaded, and zeroed when `zero` (the
// caller's: the other cap is off, so nobody's depth is lost).  The caller has set the device; the stream is idle.
int cover_track_up(sfa_session *s, const bool zero) {
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    const CoverModel cm(s);
    std::vector<int64_t> cov_off;
    sfa::coverage_offsets(cm.ref_len.data(), c->model.num_ref, &cov_off);
    const bool fresh = !v.has_track();
    if (int rc = v.reserve_track(cov_off.back(), c->model.num_ref)) return rc;
    if (int rc = sess::create_events(v.ev, 2)) return rc;
    v.h_cov_off.swap(cov_off);
    HIP_TRY(hipMemcpyAsync(v.d_cov_off.p, v.h_cov_off.data(), 8 * v.h_cov_off.size(), hipMemcpyHostToDevice, c->stream));
    if (zero || fresh) HIP_TRY(hipMemsetAsync(v.d_depth.p, 0, 4 * static_cast<size_t>(v.h_cov_off.back()), c->stream));
    return SFA_OK;
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

// ---- target classes (target_rules.hpp, sdtw_session_class.hpp) ----

int sfa_session_targets(sfa_session_t *s, const sfa_target_t *targets, int32_t n) {
    static const char *const who = "sfa_session_targets";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->resweep)
        return fail(SFA_EINVAL, "%s: the session was created with SFA_SESSION_RESWEEP: its carried row belongs to the reversed query, and what its minimum means has "
                                "not been looked into",
                    who);
    if (s->spread) {  // every sub-session holds the mask (no slot needs to be empty: spread_config's check does not apply)
        if (int rc = spread_live(s, who)) return rc;
        sess::Spread &sp = *s->spread;
        std::vector<int> rcs(sp.subs.size(), 0);
        const int rc = sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = sfa_session_targets(sp.subs[r], targets, n)) : static_cast<int>(SFA_OK); });
        size_t have = 0, failed = 0;
        for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
        if (failed != 0 && failed != have) sp.broken = true;
        return rc;
    }
    sfa_ctx *c = s->c;
    sess::Targets &t = s->targets;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a mask in use is not replaced under a kernel)
    if (n == 0) {
        t.on = false;
        t.on_cols = 0;
        t.first_on = t.first_off = -1;
        std::vector<uint32_t>().swap(t.h_mask);
        t.d_mask = DevBuf{};  // (freed; the buffers of a call stay for the next mask)
        s->reach.free_all();  // (a reach list's anchors go with its mask)
        cover_drop_mask(s);  // (a coverage cap lives on the mask: off with it; a group cap keeps the depth track)
        return SFA_OK;
    }
    if (c->model.total_cols >= INT32_MAX) return fail(SFA_ERANGE, "%s: the reference has %lld columns; the classes count them in 31 bits", who, (long long)c->model.total_cols);
    // the model's tables on the host: jobs are contig-major, '+' before '-' (sfa_context.hip)
    const int32_t nj = c->model.n_jobs, strands = nj / c->model.num_ref;
    std::vector<int32_t> job_contig(nj), ref_len(c->model.num_ref);
    std::vector<int8_t> job_strand(nj);
    for (int32_t j = 0; j < nj; ++j) job_contig[j] = j / strands, job_strand[j] = (j % strands) ? '-' : '+';
    for (int32_t r = 0; r < c->model.num_ref; ++r) ref_len[r] = c->model.h_job_len[static_cast<size_t>(r) * strands];
    const sfa::TargetModel m{c->model.num_ref, nj, job_contig.data(), job_strand.data(), c->model.h_job_len.data(), s->rows.h_col_off.data(), ref_len.data(),
                             c->model.h_ref_off.data(), c->model.total_cols};
    char msg[192];
    if (sfa::target_list_error(targets, n, m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    std::vector<uint32_t> mask;
    const int64_t on_cols = sfa::target_mask(targets, n, m, &mask);
    if (int rc = t.reserve(c->model.total_cols)) return rc;
    if (int rc = sess::create_events(t.ev, 2)) return rc;
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

// ---- reach targets (reach_rules.hpp, sdtw_session_reach.hpp) ----

size_t sfa_session_reach_bytes(const sfa_ref_t *ref, int flag) {
    if (!ref || ref->num_ref <= 0 || !ref->ref_lengths) return 0;
    int64_t cols = 0;
    for (int32_t r = 0; r < ref->num_ref; ++r) {
        if (ref->ref_lengths[r] <= 0) return 0;
        cols += static_cast<int64_t>(ref->ref_lengths[r]) * ((flag & SFA_RNA) ? 1 : 2);
    }
    return sfa::reach_bytes(cols);
}

int sfa_session_targets_reach(sfa_session_t *s, const sfa_reach_target_t *targets, int32_t n) {
    static const char *const who = "sfa_session_targets_reach";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->resweep)
        return fail(SFA_EINVAL, "%s: the session was created with SFA_SESSION_RESWEEP: its carried row belongs to the reversed query, and what its minimum means has "
                                "not been looked into",
                    who);
    if (n == 0) return sfa_session_targets(s, nullptr, 0);  // (targets off, the anchors freed: one path)
    if (s->spread) {  // every sub-session holds the mask and the anchors, as in sfa_session_targets
        if (int rc = spread_live(s, who)) return rc;
        sess::Spread &sp = *s->spread;
        std::vector<int> rcs(sp.subs.size(), 0);
        const int rc = sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = sfa_session_targets_reach(sp.subs[r], targets, n)) : static_cast<int>(SFA_OK); });
        size_t have = 0, failed = 0;
        for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
        if (failed != 0 && failed != have) sp.broken = true;
        return rc;
    }
    sfa_ctx *c = s->c;
    sess::Targets &t = s->targets;
    sess::Reach &rc_ = s->reach;
    if (c->model.total_cols >= INT32_MAX) return fail(SFA_ERANGE, "%s: the reference has %lld columns; the classes count them in 31 bits", who, (long long)c->model.total_cols);
    const CoverModel cm(s);
    char msg[224];
    if (sfa::reach_list_error(targets, n, cm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    sfa::ReachPrepared prep;
    sfa::reach_prepare(targets, n, cm.m, &prep);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a mask in use is not replaced under a kernel)
    // (from here on the old mask is gone: an allocation or device failure leaves the session without targets -- and so without a
    // mask cap, which lives on the mask -- never with half of two lists; include/sigfish_amd.h says so)
    const auto give_up = [&](int rc) {
        sfa_session_targets(s, nullptr, 0);
        return rc;
    };
    if (int rc = t.reserve(c->model.total_cols)) return give_up(rc);
    if (int rc = sess::create_events(t.ev, 2)) return give_up(rc);
    if (int rc = rc_.reserve(c->model.total_cols, prep.runs.size(), c->model.n_jobs)) return give_up(rc);
    hipStream_t st = c->stream;
    const size_t words = sfa::target_mask_words(c->model.total_cols);
    sfa::CoverStats *hs = rc_.h_stats.as<sfa::CoverStats>();
    hs[0] = sfa::CoverStats{0ull, sfa::kNoColumn, sfa::kNoColumn};
    sfa::SessionReachBuildArgs a;
    a.runs = rc_.d_runs.as<sfa::ReachRun>();
    a.run_off = rc_.d_run_off.as<int32_t>();
    a.col_off = s->rows.d_col_off.as<int64_t>();
    a.mask = t.d_mask.as<uint32_t>();
    a.anchor = rc_.d_anchor.as<int32_t>();
    a.stats = rc_.d_stats.as<sfa::CoverStats>();
    a.total_cols = c->model.total_cols;
    a.n_jobs = c->model.n_jobs;
    a.n_words = static_cast<int32_t>(words);
    const auto enqueue = [&]() -> int {  // (the uploads read pageable memory: they are through when the calls return)
        HIP_TRY(hipMemcpyAsync(rc_.d_stats.p, hs, sizeof(sfa::CoverStats), hipMemcpyHostToDevice, st));
        if (!prep.runs.empty()) HIP_TRY(hipMemcpyAsync(rc_.d_runs.p, prep.runs.data(), sizeof(sfa::ReachRun) * prep.runs.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(rc_.d_run_off.p, prep.run_off.data(), 4 * prep.run_off.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(t.d_mask.p, 0, 4 * words, st));  // (the spare word stays zero)
        hipLaunchKernelGGL(sfa::session_reach_build_kernel, dim3(sfa::cover_mask_blocks(c->model.total_cols)), dim3(sfa::kCoverThreads), 0, st, a);
        KERNEL_TRY();
        HIP_TRY(hipMemcpyAsync(hs + 1, rc_.d_stats.p, sizeof(sfa::CoverStats), hipMemcpyDeviceToHost, st));
        return SFA_OK;
    };
    if (int rc = enqueue()) return give_up(rc);
    if (hipStreamSynchronize(st) != hipSuccess) return give_up(fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError())));
    rc_.d_runs = DevBuf{}, rc_.d_run_off = DevBuf{};  // (the runs were the call's: only the anchors and the 16-byte record stay)
    std::vector<uint32_t>().swap(t.h_mask);  // (the mask was built on the device: sfa_session_reach_tables copies it back)
    t.on_cols = static_cast<int64_t>(hs[1].live);
    t.first_on = hs[1].first_on == sfa::kNoColumn ? -1 : hs[1].first_on;
    t.first_off = hs[1].first_off == sfa::kNoColumn ? -1 : hs[1].first_off;
    t.on = true;
    rc_.on = true;
    if (s->cover.on()) return cover_derive(s, who);  // (the depth is kept: the live mask of the new base mask and its anchors)
    return SFA_OK;
}

int sfa_session_reach_tables(sfa_session_t *s, uint32_t *mask, size_t n_words, int32_t *anchor, int64_t n_cols) {
    static const char *const who = "sfa_session_reach_tables";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (s->spread) {
        if (int rc = spread_live(s, who)) return rc;
        return sfa_session_reach_tables(s->spread->subs[0], mask, n_words, anchor, n_cols);  // (shard 0 answers: every shard holds the same tables)
    }
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

int64_t sfa_session_target_columns(sfa_session_t *s) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_target_columns: null session");
    if (s->spread) return sfa_session_target_columns(s->spread->subs[0]);  // (sub-session 0 always exists, as in spread_classes)
    if (s->cover.on()) return s->cover.live_cols;
    return s->targets.on ? s->targets.on_cols : 0;
}

int sfa_session_classes(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_class_t *out) {
    static const char *const who = "sfa_session_classes";
    if (!s || n < 0 || (n > 0 && (!slot || !out))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->spread) return spread_classes(s, slot, n, out);
    sess::Targets &t = s->targets;
    if (!t.on) return fail(SFA_EINVAL, "%s: the session has no targets (sfa_session_targets)", who);
    if (int rc = check_slots(s, slot, n, who)) return rc;
    begin_call(s);  // (the stamps say which slots this call has named)
    for (int32_t i = 0; i < n; ++i)
        if (int rc = claim_slot(s, slot[i], who)) return rc;
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    sfa_class_t none{};
    none.on_score = none.off_score = INFINITY;
    none.on_rid = none.on_pos_end = none.off_rid = none.off_pos_end = -1;
    t.live.clear();
    for (int32_t i = 0; i < n; ++i)  // empty and poisoned slots are not launched
        if (!s->rows.poison[slot[i]] && s->rows.len[slot[i]] > 0) t.live.push_back(i);
    const int32_t m = static_cast<int32_t>(t.live.size()), parts = sfa::class_parts(c->model.total_cols);
    // (every refusal in front of the first write to the caller's records)
    if (static_cast<int64_t>(m) * parts > INT32_MAX) return fail(SFA_ERANGE, "%s: %d slots x %d parts of a row are more blocks than a launch takes", who, m, parts);
    if (m > 0)
        if (int rc = t.reserve_call(static_cast<size_t>(m), static_cast<size_t>(parts))) return rc;
    for (int32_t i = 0; i < n; ++i) out[i] = none;
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    if (m > 0) {
        int32_t *hs = t.h_slot.as<int32_t>();
        for (int32_t k = 0; k < m; ++k) hs[k] = slot[t.live[k]];
        hipStream_t st = c->stream;
        HIP_TRY(hipMemcpyAsync(t.d_slot.p, hs, 4 * static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        sfa::SessionClassArgs a;
        a.slot = t.d_slot.as<int32_t>();
        a.rows = s->rows.d_row_c.as<float>() + sfa::kSessionPad;
        a.mask = s->cover.on() ? s->cover.d_live.as<uint32_t>() : t.d_mask.as<uint32_t>();  // (the kernel is the same: another pointer)
        a.part = t.d_part.as<sfa::ClassPartial>();
        a.total_cols = c->model.total_cols;
        a.n = m;
        a.n_parts = parts;
        sfa::SessionClassRowsArgs ra;
        ra.part = a.part;
        ra.col_off = s->rows.d_col_off.as<int64_t>();
        ra.ref = c->model.tables();
        ra.out = t.d_cls.as<sfa_class_t>();
        ra.n = m;
        ra.n_parts = parts;
        ra.n_jobs = c->model.n_jobs;
        ra.first_on = s->cover.on() ? s->cover.first_on : t.first_on;
        ra.first_off = s->cover.on() ? s->cover.first_off : t.first_off;
        HIP_TRY(hipEventRecord(t.ev[0], st));
        hipLaunchKernelGGL(sfa::sdtw_session_class_kernel, dim3(static_cast<unsigned>(m) * parts), dim3(sfa::kClassThreads), 0, st, a);
        KERNEL_TRY();
        hipLaunchKernelGGL(sfa::sdtw_session_class_rows_kernel, dim3(m), dim3(64), 0, st, ra);
        KERNEL_TRY();
        HIP_TRY(hipEventRecord(t.ev[1], st));
        HIP_TRY(hipMemcpyAsync(t.h_cls.p, t.d_cls.p, sizeof(sfa_class_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        pr.class_ms = pr.total_ms = ms;
        for (int32_t k = 0; k < m; ++k) {
            out[t.live[k]] = t.h_cls.as<sfa_class_t>()[k];
            out[t.live[k]].n_events = static_cast<int32_t>(s->rows.len[slot[t.live[k]]]);
        }
    }
    c->prof = pr;
    return SFA_OK;
}

int sfa_target_decide(const sfa_class_t *cls, int32_t mode, int32_t min_events, float margin) {
    return cls ? sfa::target_decide(*cls, mode, min_events, margin) : 0;
}

// ---- coverage caps (coverage_rules.hpp, sdtw_session_cover.hpp) ----

size_t sfa_session_coverage_bytes(const sfa_ref_t *ref, int flag) {
    if (!ref || ref->num_ref <= 0 || !ref->ref_lengths) return 0;
    int64_t entries = 0, cols = 0;
    for (int32_t r = 0; r < ref->num_ref; ++r) {
        if (ref->ref_lengths[r] <= 0) return 0;
        entries += sfa::coverage_track_len(ref->ref_lengths[r]);
        cols += static_cast<int64_t>(ref->ref_lengths[r]) * ((flag & SFA_RNA) ? 1 : 2);
    }
    return sfa::coverage_bytes(entries, cols);
}

int sfa_session_coverage_config(sfa_session_t *s, int32_t cap) {
    static const char *const who = "sfa_session_coverage_config";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (cap < 0 || cap > sfa::kCoverCapMax) return fail(SFA_EINVAL, "%s: cap must be 0 (off) .. %d, not %d", who, sfa::kCoverCapMax, cap);
    if (s->spread) {
        if (int rc = spread_live(s, who)) return rc;
        if (cap > 0 && !s->spread->subs[0]->targets.on) return fail(SFA_EINVAL, "%s: the session has no targets (sfa_session_targets)", who);
        return cover_spread_all(s, who, [&](sfa_session *sub) { return sfa_session_coverage_config(sub, cap); });
    }
    sfa_ctx *c = s->c;
    sess::Coverage &v = s->cover;
    if (cap > 0 && !s->targets.on) return fail(SFA_EINVAL, "%s: the session has no targets (sfa_session_targets)", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a mask in use is not replaced under a kernel)
    if (cap == 0) {
        cover_drop_mask(s);
        return SFA_OK;
    }
    if (int rc = cover_track_up(s, !s->gcover.on())) return rc;  // (a group cap's depth is kept: the track is the session's one)
    if (int rc = v.reserve_mask(c->model.total_cols)) {
        cover_drop_mask(s);
        return rc;
    }
    HIP_TRY(hipMemsetAsync(v.d_live.p, 0, 4 * sfa::target_mask_words(c->model.total_cols), c->stream));  // (the spare word stays zero)
    v.cap = cap;
    if (int rc = cover_derive(s, who)) {  // (without a group cap the depth is 0 everywhere: the live mask is the base mask)
        cover_drop_mask(s);
        return rc;
    }
    return SFA_OK;
}

int sfa_session_coverage_add(sfa_session_t *s, const sfa_target_t *iv, int32_t n, int64_t *open_columns) {
    static const char *const who = "sfa_session_coverage_add";
    if (!s || n < 0 || (n > 0 && !iv)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (n > sfa::kCoverIntervalsMax) return fail(SFA_EINVAL, "%s: %d intervals in one call; at most %d", who, n, sfa::kCoverIntervalsMax);
    sfa_session *first = s->spread ? s->spread->subs[0] : s;  // (sub-session 0 always exists; every sub-session holds the same state)
    if (s->spread)
        if (int rc = spread_live(s, who)) return rc;
    if (!first->cover.on() && !first->gcover.on()) return fail(SFA_EINVAL, "%s: the session has no coverage cap (sfa_session_coverage_config)", who);
    {
        const CoverModel cm(first);
        char msg[192];
        if (sfa::coverage_list_error(iv, n, cm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    }
    if (s->spread) {
        if (int rc = cover_spread_all(s, who, [&](sfa_session *sub) { return sfa_session_coverage_add(sub, iv, n, nullptr); })) return rc;
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
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    pr.class_ms = pr.total_ms = v.ms;
    c->prof = pr;
    if (open_columns) *open_columns = sfa_session_target_columns(s);  // (the live columns under a mask cap; without one the mask's own)
    return SFA_OK;
}

int sfa_session_coverage_depth(sfa_session_t *s, int32_t contig, uint32_t *out, int32_t n) {
    static const char *const who = "sfa_session_coverage_depth";
    if (!s || !out) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->spread) {
        if (int rc = spread_live(s, who)) return rc;
        return sfa_session_coverage_depth(s->spread->subs[0], contig, out, n);  // (shard 0 answers, on the caller's thread as in for_each_shard)
    }
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
    if (!ref || ref->num_ref <= 0 || !ref->ref_lengths || n_groups < 1 || n_groups > sfa::kGroupMax) return 0;
    int64_t entries = 0, cols = 0;
    for (int32_t r = 0; r < ref->num_ref; ++r) {
        if (ref->ref_lengths[r] <= 0) return 0;
        entries += sfa::coverage_track_len(ref->ref_lengths[r]);
        cols += static_cast<int64_t>(ref->ref_lengths[r]) * ((flag & SFA_RNA) ? 1 : 2);
    }
    return 4 * static_cast<size_t>(entries) + sess::GroupCover::bytes(cols, n_groups);
}

int sfa_session_group_coverage_config(sfa_session_t *s, int32_t cap) {
    static const char *const who = "sfa_session_group_coverage_config";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (cap < 0 || cap > sfa::kGroupCapMax) return fail(SFA_EINVAL, "%s: cap must be 0 (off) .. %d, not %d", who, sfa::kGroupCapMax, cap);
    if (s->spread) {
        if (int rc = spread_live(s, who)) return rc;
        if (cap > 0 && !s->spread->subs[0]->groups.on()) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
        return cover_spread_all(s, who, [&](sfa_session *sub) { return sfa_session_group_coverage_config(sub, cap); });
    }
    sfa_ctx *c = s->c;
    sess::GroupCover &gc = s->gcover;
    if (cap > 0 && !s->groups.on()) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a table in use is not replaced under a kernel)
    if (cap == 0) {
        gcover_drop(s);
        return SFA_OK;
    }
    // (a mask cap's depth is kept: the track is the session's one.  Whatever fails from here on leaves the group cap off)
    int rc = cover_track_up(s, !s->cover.on());
    if (!rc) rc = gc.reserve(c->model.total_cols, s->groups.n_groups);
    if (!rc) rc = sess::create_events(gc.ev, 2);
    if (rc) {
        gcover_drop(s);
        return rc;
    }
    gc.cap = cap;
    if (int rc = gcover_derive(s, who)) {
        gcover_drop(s);
        return rc;
    }
    return SFA_OK;
}

int sfa_session_group_coverage(sfa_session_t *s, sfa_group_cover_t *out, int32_t n) {
    static const char *const who = "sfa_session_group_coverage";
    if (!s || !out) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->spread) {
        if (int rc = spread_live(s, who)) return rc;
        return sfa_session_group_coverage(s->spread->subs[0], out, n);  // (shard 0 answers: every shard holds the same tables and tracks)
    }
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
    if (s->greach.on) {  // (a reach label table: the '+' jobs' body columns only)
        sfa::SessionReachLabelGroupArgs a;
        a.base = s->groups.d_label.as<uint64_t>();
        a.anchor = s->greach.d_anchor.as<int32_t>();
        a.depth = s->cover.d_depth.as<uint32_t>();
        a.cov_off = s->cover.d_cov_off.as<int64_t>();
        a.col_off = s->rows.d_col_off.as<int64_t>();
        a.ref = c->model.tables();
        a.rec = gc.d_rec.as<sfa_group_cover_t>();
        a.total_cols = c->model.total_cols;
        a.n_jobs = c->model.n_jobs;
        a.n_groups = s->groups.n_groups;
        a.cap = static_cast<uint32_t>(gc.cap);
        hipLaunchKernelGGL(sfa::session_reach_label_group_kernel, dim3(sfa::group_cover_blocks(c->model.total_cols)), dim3(sfa::kGroupCoverThreads), 0, st, a);
        KERNEL_TRY();
    } else {
        sfa::SessionCoverGroupArgs a;
        a.base = s->groups.d_label.as<uint64_t>();
        a.depth = s->cover.d_depth.as<uint32_t>();
        a.cov_off = s->cover.d_cov_off.as<int64_t>();
        a.col_off = s->rows.d_col_off.as<int64_t>();
        a.ref = c->model.tables();
        a.rec = gc.d_rec.as<sfa_group_cover_t>();
        a.total_cols = c->model.total_cols;
        a.n_jobs = c->model.n_jobs;
        a.n_groups = s->groups.n_groups;
        a.cap = static_cast<uint32_t>(gc.cap);
        hipLaunchKernelGGL(sfa::session_cover_group_kernel, dim3(sfa::group_cover_blocks(c->model.total_cols)), dim3(sfa::kGroupCoverThreads), 0, st, a);
        KERNEL_TRY();
    }
    HIP_TRY(hipEventRecord(gc.ev[1], st));
    HIP_TRY(hipMemcpyAsync(hr + entries, gc.d_rec.p, sizeof(sfa_group_cover_t) * static_cast<size_t>(entries), hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, gc.ev[0], gc.ev[1]));
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    pr.class_ms = pr.total_ms = ms;
    c->prof = pr;
    memcpy(out, hr + entries, sizeof(sfa_group_cover_t) * static_cast<size_t>(entries));
    return SFA_OK;
}

// ---- target groups (group_rules.hpp, sdtw_session_group.hpp) ----

int sfa_session_target_groups(sfa_session_t *s, const sfa_group_target_t *targets, int32_t n, int32_t n_groups) {
    static const char *const who = "sfa_session_target_groups";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->resweep)
        return fail(SFA_EINVAL, "%s: the session was created with SFA_SESSION_RESWEEP: its carried row belongs to the reversed query, and what its minimum means has "
                                "not been looked into",
                    who);
    if (s->spread) {  // every sub-session holds the table (no slot needs to be empty: spread_config's check does not apply)
        if (int rc = spread_live(s, who)) return rc;
        sess::Spread &sp = *s->spread;
        std::vector<int> rcs(sp.subs.size(), 0);
        const int rc = sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = sfa_session_target_groups(sp.subs[r], targets, n, n_groups)) : static_cast<int>(SFA_OK); });
        size_t have = 0, failed = 0;
        for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
        if (failed != 0 && failed != have) sp.broken = true;
        return rc;
    }
    sfa_ctx *c = s->c;
    sess::Groups &g = s->groups;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a table in use is not replaced under a kernel)
    s->open.first.clear();                     // (sfa_session_open_classes looks for the labels' first columns again)
    if (n == 0) {
        g.n_groups = 0;
        std::vector<uint16_t>().swap(g.h_label);
        g.d_label = DevBuf{};  // (freed; the buffers of a call stay for the next table)
        s->greach.free_all();  // (a reach list's group anchors go with its label table)
        if (s->gcover.on()) gcover_drop(s);  // (a group cap lives on the labels: off with them)
        return SFA_OK;
    }
    if (c->model.total_cols >= INT32_MAX) return fail(SFA_ERANGE, "%s: the reference has %lld columns; the groups count them in 31 bits", who, (long long)c->model.total_cols);
    // the model's tables on the host: jobs are contig-major, '+' before '-' (sfa_context.hip)
    const int32_t nj = c->model.n_jobs, strands = nj / c->model.num_ref;
    std::vector<int32_t> job_contig(nj), ref_len(c->model.num_ref);
    std::vector<int8_t> job_strand(nj);
    for (int32_t j = 0; j < nj; ++j) job_contig[j] = j / strands, job_strand[j] = (j % strands) ? '-' : '+';
    for (int32_t r = 0; r < c->model.num_ref; ++r) ref_len[r] = c->model.h_job_len[static_cast<size_t>(r) * strands];
    const sfa::TargetModel m{c->model.num_ref, nj, job_contig.data(), job_strand.data(), c->model.h_job_len.data(), s->rows.h_col_off.data(), ref_len.data(),
                             c->model.h_ref_off.data(), c->model.total_cols};
    char msg[256];
    if (sfa::group_list_error(targets, n, n_groups, m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    std::vector<uint16_t> label;
    sfa::group_labels(targets, n, n_groups, m, &label);
    if (int rc = g.reserve(c->model.total_cols)) return rc;
    if (int rc = sess::create_events(g.ev, 2)) return rc;
    if (s->gcover.on())  // (the live table's tables follow the new n_groups; a group cap never outlives a failure here)
        if (int rc = s->gcover.reserve(c->model.total_cols, n_groups)) {
            gcover_drop(s);
            return rc;
        }
    g.n_groups = 0;  // (off until the new table is up)
    s->greach.free_all();  // (a plain table replaces a reach list, before the table is overwritten: no anchor outlives the table it belongs to)
    g.h_label.swap(label);
    const auto upload = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(g.d_label.p, g.h_label.data(), 2 * g.h_label.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SFA_OK;
    };
    if (int rc = upload()) {
        if (s->gcover.on()) gcover_drop(s);  // (no groups: no group cap)
        return rc;
    }
    g.n_groups = n_groups;
    if (s->gcover.on()) {  // (the depth is kept: the live table of the new base table)
        const int rc = gcover_derive(s, who);
        if (rc) gcover_drop(s);
        return rc;
    }
    return SFA_OK;
}

// ---- reach groups (reach_group_rules.hpp, sdtw_session_reachgroup.hpp) ----

size_t sfa_session_group_reach_bytes(const sfa_ref_t *ref, int flag) {
    if (!ref || ref->num_ref <= 0 || !ref->ref_lengths) return 0;
    int64_t cols = 0;
    for (int32_t r = 0; r < ref->num_ref; ++r) {
        if (ref->ref_lengths[r] <= 0) return 0;
        cols += static_cast<int64_t>(ref->ref_lengths[r]) * ((flag & SFA_RNA) ? 1 : 2);
    }
    return sfa::reach_group_bytes(cols);
}

int sfa_session_target_groups_reach(sfa_session_t *s, const sfa_reach_group_target_t *targets, int32_t n, int32_t n_groups) {
    static const char *const who = "sfa_session_target_groups_reach";
    if (!s || n < 0 || (n > 0 && !targets)) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->resweep)
        return fail(SFA_EINVAL, "%s: the session was created with SFA_SESSION_RESWEEP: its carried row belongs to the reversed query, and what its minimum means has "
                                "not been looked into",
                    who);
    if (n == 0) return sfa_session_target_groups(s, nullptr, 0, n_groups);  // (groups off, the anchors freed: one path)
    if (s->spread) {  // every sub-session holds the table and its anchors, as in sfa_session_target_groups
        if (int rc = spread_live(s, who)) return rc;
        sess::Spread &sp = *s->spread;
        std::vector<int> rcs(sp.subs.size(), 0);
        const int rc =
            sfa::for_each_shard(s->c, [&](size_t r) { return sp.subs[r] ? (rcs[r] = sfa_session_target_groups_reach(sp.subs[r], targets, n, n_groups)) : static_cast<int>(SFA_OK); });
        size_t have = 0, failed = 0;
        for (size_t r = 0; r < sp.subs.size(); ++r) have += sp.subs[r] != nullptr, failed += rcs[r] != SFA_OK;
        if (failed != 0 && failed != have) sp.broken = true;
        return rc;
    }
    sfa_ctx *c = s->c;
    sess::Groups &g = s->groups;
    sess::GroupReach &gr = s->greach;
    if (c->model.total_cols >= INT32_MAX) return fail(SFA_ERANGE, "%s: the reference has %lld columns; the groups count them in 31 bits", who, (long long)c->model.total_cols);
    const CoverModel cm(s);
    char msg[256];
    if (sfa::reach_group_list_error(targets, n, n_groups, cm.m, msg, sizeof msg)) return fail(SFA_EINVAL, "%s: %s", who, msg);
    sfa::ReachGroupPrepared prep;
    sfa::reach_group_prepare(targets, n, cm.m, &prep);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (a table in use is not replaced under a kernel)
    // (from here on the old table is gone: an allocation or device failure leaves the session without groups -- and so without a
    // group cap, which lives on the labels -- never with half of two lists; include/sigfish_amd.h says so)
    const auto give_up = [&](int rc) {
        sfa_session_target_groups(s, nullptr, 0, 0);
        return rc;
    };
    s->open.first.clear();
    g.n_groups = 0;  // (off until the new table is up)
    std::vector<uint16_t>().swap(g.h_label);  // (the table is built on the device: sfa_session_group_reach_tables copies it back)
    gr.on = false;
    if (int rc = g.reserve(c->model.total_cols)) return give_up(rc);
    if (int rc = sess::create_events(g.ev, 2)) return give_up(rc);
    if (int rc = gr.reserve(c->model.total_cols, prep.runs.size(), c->model.n_jobs, n_groups)) return give_up(rc);
    if (s->gcover.on())  // (the live table's tables follow the new n_groups)
        if (int rc = s->gcover.reserve(c->model.total_cols, n_groups)) return give_up(rc);
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
    const auto enqueue = [&]() -> int {  // (the uploads of the runs read pageable memory: they are through when the calls return)
        HIP_TRY(hipMemcpyAsync(gr.d_first.p, hf, 4 * entries, hipMemcpyHostToDevice, st));
        if (!prep.runs.empty()) HIP_TRY(hipMemcpyAsync(gr.d_runs.p, prep.runs.data(), sizeof(sfa::ReachGroupRun) * prep.runs.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(gr.d_run_off.p, prep.run_off.data(), 4 * prep.run_off.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(g.d_label.as<uint16_t>() + tail), static_cast<unsigned short>(n_groups), n_tail, st));
        hipLaunchKernelGGL(sfa::session_reach_label_build_kernel, dim3(sfa::group_cover_blocks(c->model.total_cols)), dim3(sfa::kGroupCoverThreads), 0, st, a);
        KERNEL_TRY();
        HIP_TRY(hipMemcpyAsync(hf + entries, gr.d_first.p, 4 * entries, hipMemcpyDeviceToHost, st));
        return SFA_OK;
    };
    if (int rc = enqueue()) return give_up(rc);
    if (hipStreamSynchronize(st) != hipSuccess) return give_up(fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError())));
    sfa::group_cover_firsts_for_open(hf + entries, n_groups, &s->open.first);  // (what sfa_session_open_classes needs once per label table)
    gr.free_call();  // (the runs and the firsts were the call's: only the anchors stay)
    g.n_groups = n_groups;
    gr.on = true;
    if (s->gcover.on()) {  // (the depth is kept: the live table of the new base table and its anchors)
        const int rc = gcover_derive(s, who);
        if (rc) return give_up(rc);
    }
    return SFA_OK;
}

int sfa_session_group_reach_tables(sfa_session_t *s, uint16_t *label, int32_t *anchor, int64_t n_cols) {
    static const char *const who = "sfa_session_group_reach_tables";
    if (!s) return fail(SFA_EINVAL, "%s: null session", who);
    if (s->spread) {
        if (int rc = spread_live(s, who)) return rc;
        return sfa_session_group_reach_tables(s->spread->subs[0], label, anchor, n_cols);  // (shard 0 answers: every shard holds the same tables)
    }
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

int32_t sfa_session_group_count(sfa_session_t *s) {
    if (!s) return fail(SFA_EINVAL, "sfa_session_group_count: null session");
    if (s->spread) return sfa_session_group_count(s->spread->subs[0]);  // (sub-session 0 always exists, as in spread_classes)
    return s->groups.n_groups;
}

int sfa_session_group_bests(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_group_best_t *bests, sfa_group_head_t *heads) {
    static const char *const who = "sfa_session_group_bests";
    if (!s || n < 0 || (n > 0 && (!slot || !heads))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->spread) return spread_group_bests(s, slot, n, bests, heads);
    sess::Groups &g = s->groups;
    if (!g.on()) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (int rc = check_slots(s, slot, n, who)) return rc;
    begin_call(s);  // (the stamps say which slots this call has named)
    for (int32_t i = 0; i < n; ++i)
        if (int rc = claim_slot(s, slot[i], who)) return rc;
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    g.live.clear();
    for (int32_t i = 0; i < n; ++i)  // empty and poisoned slots are not launched
        if (!s->rows.poison[slot[i]] && s->rows.len[slot[i]] > 0) g.live.push_back(i);
    const int32_t m = static_cast<int32_t>(g.live.size()), parts = sfa::class_parts(c->model.total_cols), entries = g.n_groups + 1;
    // (every refusal in front of the first write to the caller's records)
    if (static_cast<int64_t>(m) * parts > INT32_MAX) return fail(SFA_ERANGE, "%s: %d slots x %d parts of a row are more blocks than a launch takes", who, m, parts);
    if (m > 0)
        if (int rc = g.reserve_call(static_cast<size_t>(m), static_cast<size_t>(entries), bests != nullptr)) return rc;
    sfa_group_best_t no_best{};
    no_best.score = INFINITY;
    no_best.rid = no_best.pos_end = -1;
    for (int32_t i = 0; i < n; ++i) heads[i] = sfa::group_head_none();
    if (bests)
        for (size_t k = 0; k < static_cast<size_t>(n) * entries; ++k) bests[k] = no_best;
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    if (m > 0) {
        int32_t *hs = g.h_slot.as<int32_t>();
        for (int32_t k = 0; k < m; ++k) hs[k] = slot[g.live[k]];
        hipStream_t st = c->stream;
        const size_t n_keys = static_cast<size_t>(m) * entries;
        HIP_TRY(hipMemcpyAsync(g.d_slot.p, hs, 4 * static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        sfa::SessionGroupArgs a;
        a.slot = g.d_slot.as<int32_t>();
        a.rows = s->rows.d_row_c.as<float>() + sfa::kSessionPad;
        a.label = s->gcover.on() ? s->gcover.d_live.as<uint64_t>() : g.d_label.as<uint64_t>();  // (the kernel is the same: another pointer)
        a.key = g.d_key.as<unsigned long long>();
        a.total_cols = c->model.total_cols;
        a.n = m;
        a.n_parts = parts;
        a.n_entries = entries;
        sfa::SessionGroupRowsArgs ra;
        ra.key = a.key;
        ra.col_off = s->rows.d_col_off.as<int64_t>();
        ra.ref = c->model.tables();
        ra.best = bests ? g.d_best.as<sfa_group_best_t>() : nullptr;
        ra.head = g.d_head.as<sfa_group_head_t>();
        ra.n = m;
        ra.n_entries = entries;
        ra.n_jobs = c->model.n_jobs;
        HIP_TRY(hipEventRecord(g.ev[0], st));
        HIP_TRY(hipMemsetAsync(g.d_key.p, 0xff, 8 * n_keys, st));  // all-ones: no column met
        hipLaunchKernelGGL(sfa::sdtw_session_group_kernel, dim3(static_cast<unsigned>(m) * parts), dim3(sfa::kClassThreads), 0, st, a);
        KERNEL_TRY();
        hipLaunchKernelGGL(sfa::sdtw_session_group_rows_kernel, dim3(m), dim3(64), 0, st, ra);
        KERNEL_TRY();
        HIP_TRY(hipEventRecord(g.ev[1], st));
        HIP_TRY(hipMemcpyAsync(g.h_head.p, g.d_head.p, sizeof(sfa_group_head_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        if (bests) HIP_TRY(hipMemcpyAsync(g.h_best.p, g.d_best.p, sizeof(sfa_group_best_t) * n_keys, hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
        pr.class_ms = pr.total_ms = ms;
        for (int32_t k = 0; k < m; ++k) {
            heads[g.live[k]] = g.h_head.as<sfa_group_head_t>()[k];
            heads[g.live[k]].n_events = static_cast<int32_t>(s->rows.len[slot[g.live[k]]]);
            if (bests) memcpy(bests + static_cast<size_t>(g.live[k]) * entries, g.h_best.as<sfa_group_best_t>() + static_cast<size_t>(k) * entries, sizeof(sfa_group_best_t) * entries);
        }
    }
    c->prof = pr;
    return SFA_OK;
}

int sfa_group_decide(const sfa_group_head_t *h, int32_t min_events, float margin) { return h ? sfa::group_decide(*h, min_events, margin) : -1; }

// ---- open and closed groups (quota_rules.hpp, sdtw_session_open.hpp) ----

int sfa_session_open_classes(sfa_session_t *s, const int32_t *slot, int32_t n, const uint32_t *open, int32_t n_words, sfa_open_class_t *out) {
    static const char *const who = "sfa_session_open_classes";
    if (!s || n < 0 || (n > 0 && (!slot || !out))) return fail(SFA_EINVAL, "%s: bad argument", who);
    if (s->spread) return spread_open_classes(s, slot, n, open, n_words, out);
    sess::Groups &g = s->groups;
    sess::Open &o = s->open;
    if (!g.on()) return fail(SFA_EINVAL, "%s: the session has no groups (sfa_session_target_groups)", who);
    if (open && n_words != sfa::open_words(g.n_groups))
        return fail(SFA_EINVAL, "%s: the bitmap of %d groups has %d words, not %d", who, g.n_groups, sfa::open_words(g.n_groups), n_words);
    if (int rc = check_slots(s, slot, n, who)) return rc;
    begin_call(s);  // (the stamps say which slots this call has named)
    for (int32_t i = 0; i < n; ++i)
        if (int rc = claim_slot(s, slot[i], who)) return rc;
    if (n == 0) return SFA_OK;
    sfa_ctx *c = s->c;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    o.live.clear();
    for (int32_t i = 0; i < n; ++i)  // empty and poisoned slots are not launched
        if (!s->rows.poison[slot[i]] && s->rows.len[slot[i]] > 0) o.live.push_back(i);
    const int32_t m = static_cast<int32_t>(o.live.size()), parts = sfa::class_parts(c->model.total_cols);
    // (every refusal in front of the first write to the caller's records)
    if (static_cast<int64_t>(m) * parts > INT32_MAX) return fail(SFA_ERANGE, "%s: %d slots x %d parts of a row are more blocks than a launch takes", who, m, parts);
    if (m > 0) {
        if (int rc = o.reserve(static_cast<size_t>(m), static_cast<size_t>(parts))) return rc;
        if (int rc = sess::create_events(o.ev, 2)) return rc;
    }
    for (int32_t i = 0; i < n; ++i) out[i] = sfa::open_class_none();
    sfa_profile_t pr{};
    pr.segment_reruns = c->seg.seg_reruns;
    pr.blow5_fallbacks = c->blow5.blow5_fallbacks;
    if (m > 0) {
        const bool capped = s->gcover.on();  // (the live table and its firsts, which the derive left: the kernels are the same)
        if (!capped && o.first.empty()) sfa::open_label_firsts(g.h_label.data(), c->model.total_cols, g.n_groups, &o.first);
        int32_t *hs = o.h_slot.as<int32_t>();
        for (int32_t k = 0; k < m; ++k) hs[k] = slot[o.live[k]];
        hipStream_t st = c->stream;
        HIP_TRY(hipMemcpyAsync(o.d_slot.p, hs, 4 * static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        sfa::SessionOpenArgs a;
        a.slot = o.d_slot.as<int32_t>();
        a.rows = s->rows.d_row_c.as<float>() + sfa::kSessionPad;
        a.label = capped ? s->gcover.d_live.as<uint64_t>() : g.d_label.as<uint64_t>();
        a.part = o.d_part.as<sfa::ClassPartial>();
        a.total_cols = c->model.total_cols;
        a.n = m;
        a.n_parts = parts;
        sfa::open_normalise(open, g.n_groups, a.open);  // (the bitmap travels in the argument block: nothing is uploaded)
        sfa::SessionOpenRowsArgs ra;
        ra.part = a.part;
        ra.col_off = s->rows.d_col_off.as<int64_t>();
        ra.ref = c->model.tables();
        ra.label = capped ? s->gcover.d_live.as<uint16_t>() : g.d_label.as<uint16_t>();
        ra.out = o.d_out.as<sfa_open_class_t>();
        ra.n = m;
        ra.n_parts = parts;
        ra.n_jobs = c->model.n_jobs;
        sfa::open_first_cols(capped ? s->gcover.first : o.first, g.n_groups, a.open, &ra.first_on, &ra.first_off);
        HIP_TRY(hipEventRecord(o.ev[0], st));
        hipLaunchKernelGGL(sfa::sdtw_session_open_kernel, dim3(static_cast<unsigned>(m) * parts), dim3(sfa::kClassThreads), 0, st, a);
        KERNEL_TRY();
        hipLaunchKernelGGL(sfa::sdtw_session_open_rows_kernel, dim3(m), dim3(64), 0, st, ra);
        KERNEL_TRY();
        HIP_TRY(hipEventRecord(o.ev[1], st));
        HIP_TRY(hipMemcpyAsync(o.h_out.p, o.d_out.p, sizeof(sfa_open_class_t) * static_cast<size_t>(m), hipMemcpyDeviceToHost, st));
        if (hipStreamSynchronize(st) != hipSuccess) return fail(SFA_EKERNEL, "%s: the launches failed: %s", who, hipGetErrorString(hipGetLastError()));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, o.ev[0], o.ev[1]));
        pr.class_ms = pr.total_ms = ms;
        for (int32_t k = 0; k < m; ++k) {
            out[o.live[k]] = o.h_out.as<sfa_open_class_t>()[k];
            out[o.live[k]].cls.n_events = static_cast<int32_t>(s->rows.len[slot[o.live[k]]]);
        }
    }
    c->prof = pr;
    return SFA_OK;
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
