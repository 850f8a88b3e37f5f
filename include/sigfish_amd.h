/* sigfish_amd.h -- C-ABI of the MI355X-native sDTW alignment stage.
 *
 * Drop-in boundary for the reference's accelerator hook (all citations relative to hasindu2008/sigfish v0.2.0):
 *
 *   reference site                                   this library
 *   -----------------------------------------------  -----------------------------------------------
 *   init slot      src/sigfish.c:200-204 (HAVE_ACC)  sfa_init()          upload reference event arrays
 *   align_db()     src/sigfish.c:1003-1015           sfa_align_events()  whole batch, after normalise stage
 *                                                    sfa_align_batch()   same, packed SoA queries
 *   teardown slot  src/sigfish.c:221-225             sfa_destroy()
 *
 * Plain C types only (no torch / HIP types); every pointer is caller-owned unless stated.  All functions return
 * 0 on success, a negative SFA_E* code otherwise; sfa_last_error() gives the message.  Nothing here falls back to
 * a CPU implementation: without a usable gfx950 device sfa_init() fails.
 */
#ifndef SIGFISH_AMD_H
#define SIGFISH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFA_VERSION "0.1.0"

/* option bits: numerically identical to the reference's opt.flag (src/sigfish.h:30-39) so that a host can pass
 * core->opt.flag straight through.  Bits not listed are ignored. */
#define SFA_RNA 0x001 /* SIGFISH_RNA: single strand, query reversed (src/sigfish.c:860-866) */
#define SFA_DTW 0x002 /* SIGFISH_DTW: --dtw-std, standard DTW instead of subsequence (src/sigfish.c:914-917) */
#define SFA_INV 0x004 /* SIGFISH_INV: --invert, query NOT reversed for RNA */
#define SFA_REF 0x010 /* SIGFISH_REF: --full-ref (only affects how the caller built the reference arrays) */
#define SFA_END 0x020 /* SIGFISH_END: --from-end (only affects which events the caller hands over) */

enum {
    SFA_OK = 0,
    SFA_EINVAL = -1,  /* bad argument */
    SFA_ENODEV = -2,  /* no usable GPU / HIP error */
    SFA_ENOMEM = -3,  /* allocation failed */
    SFA_ERANGE = -4,  /* a size out of range (output buffer too small; sfa_plan_batch: query beyond SFA_MAX_QUERY) */
    SFA_EKERNEL = -5  /* kernel launch or execution failed (incl. an in-launch hand-over that did not arrive within "spin_limit_ms") */
};

/* Queries of up to SFA_MAX_QUERY events are held in the registers of one wavefront (two-pass kernels).  Longer ones --
 * the reference has no limit on -q (src/cdtw.c:171-189 fills whatever it is given) -- are accepted by every align entry
 * point and run as row strips of SFA_MAX_QUERY query rows each (sdtw_strips.hpp), in the same call, same rows. */
#define SFA_MAX_QUERY 2048

/* Reference event model: the fields of refsynth_t (src/sigfish.h:90-99) the alignment stage reads. */
typedef struct {
    int32_t num_ref;
    const int32_t *ref_lengths;   /* [num_ref] k-mer counts (ref->ref_lengths) */
    const int32_t *ref_st_offset; /* [num_ref] (ref->ref_st_offset) */
    const float *const *forward;  /* [num_ref][ref_lengths[i]] z-normalised expected levels */
    const float *const *reverse;  /* same for the reverse complement; NULL when SFA_RNA */
} sfa_ref_t;

/* One result row per read: the fields of aln_t (src/sigfish.h:146-158) that output formatting consumes. */
typedef struct {
    int32_t rid;     /* contig index, -1 if nothing aligned */
    int32_t pos_st;  /* after strand flip and ref_st_offset (src/sigfish.c:971-975) */
    int32_t pos_end;
    float score;     /* best   (d1) */
    float score2;    /* second (d2), +inf when there was a single candidate */
    int8_t strand;   /* '+' or '-' */
    uint8_t mapq;    /* src/sigfish.c:979-983 */
    uint8_t valid;   /* 0: read skipped (no events) -- the reference prints nothing for it */
    uint8_t pad;
} sfa_result_t;

/* The event record the reference batches hold (event_t, src/sigfish.h:57-64); used by sfa_align_events. */
typedef struct {
    uint64_t start;
    float length;
    float mean;
    float stdv;
} sfa_event_t;

typedef struct sfa_ctx sfa_ctx_t;

/* Device-side timing of the last call (HIP events recorded on the stream the kernels run on). */
typedef struct {
    double fill_ms;        /* pass 1: sdtw_fill_kernel (the dominant kernel).  A batch with queries beyond 2048 events runs their
                              row strips on streams of their own beside the other kernels: the stages then overlap, fill_ms is the
                              device time of the whole batch (= total_ms) and trace_ms is 0 */
    double trace_ms;       /* pass 2: sdtw_trace_kernel (start-column recovery of the winners) */
    double finalize_ms;    /* per-read reductions / row assembly */
    double total_ms;       /* first kernel start -> last kernel end */
    int64_t cells;         /* DP cells of the batch, algorithmic: sum(qlen) * sum over (contig,strand) of rlen */
    int64_t fill_launches; /* fill launches in the call (1) */
    int64_t ckpt_interval; /* steps between the snapshots of pass 1 in HBM (with lds_ckpt: of the sparse store) */
    int64_t ckpt_bytes;    /* HBM taken by the checkpoints of the batch */
    int64_t n_tasks;       /* wave-tasks of the fill launch */
    int64_t n_chunks;      /* pieces the (contig,strand) list was cut into */
    int64_t n_segments;    /* column segments per (contig,strand) (1: off; small batches use several, verified) */
    int64_t segment_reruns; /* batches of this context walked again because a segment hand-over did not verify */
    /* sfa_align_raw only (0 otherwise): the stages in front of the alignment, the reference's "Events time" and
     * "Normalise time" (src/sigfish.c:1026-1035) as device time */
    double events_ms;      /* pA conversion, prefix sums, t-statistics, peak picking, event statistics */
    double normalise_ms;   /* query windows: z-normalisation + packing (the window choice itself is host arithmetic) */
    /* reads of the batch whose query holds a NaN or +-inf event.  The reference aborts on such a read (assert in update_aln,
     * src/sigfish.c:611); here they are skipped: their rows come back with valid = 0. */
    int64_t non_finite_reads;
    double decode_ms;      /* sfa_align_blow5 only: record decompression (inflate), field parsing and signal decoding on the device */
    int64_t blow5_fallbacks; /* batches of this context handed to the host reader because the device declined a record */
    int64_t lds_ckpt;      /* 1: the fill kept its rolling checkpoints in LDS (ckpt_interval is then the sparse HBM store's);
                              2: and pass 2 ran inside the fill launch; 0: every snapshot went to HBM */
    int64_t trace_margin;  /* head start of pass 2 in steps (a whole query + lanes, or less: see "trace_margin") */
    int64_t fused_trace;   /* 1: pass 2 ran inside the fill launch by ticket (fill_ms covers both, trace_ms is 0) -- the LDS-checkpoint
                              fill or the 32-row fill */
    int64_t lck_fallbacks; /* with lds_ckpt: reads of the batch whose path began before the snapshot the fill saved for their winning
                              window, so that pass 2 went on to the sparse HBM store (thousands of steps each) */
    int64_t lck_from_scratch; /* with lds_ckpt: reads whose winning window is one of the first two of its strand: no snapshot, pass 2
                                 walks the strand from its start (at most two windows) */
    double class_ms;       /* sfa_session_classes only (0 otherwise): the masked reduction over the carried rows and its merge */
} sfa_profile_t;

/* How a batch is laid out on the device (host logic only; needs no GPU). */
typedef struct {
    int32_t n_quads;          /* wavefronts' worth of reads: groups of <= 4 reads with the same query length (<= 2 / 1
                                 reads for queries longer than 512 / 1024 events) */
    int32_t n_chunks;
    int32_t n_classes;        /* rows-per-lane classes present */
    int32_t max_rows_per_lane;
    int32_t ckpt_interval;
    int32_t trace_margin;
    int64_t ckpt_bytes;
    int64_t n_tasks;
    int32_t max_lanes_per_read; /* 16; 32 / 64 for queries longer than 512 / 1024 events or under lane widening */
    int32_t lane_widening;      /* 1, 2 or 4: small batches trade rows per lane for lanes per read */
} sfa_plan_info_t;

/* Create a context on HIP device `device`, copy the reference event arrays into HBM.
 * flag: SFA_* bits.  The arrays behind `ref` may be freed after the call returns. */
int sfa_init(sfa_ctx_t **ctx, const sfa_ref_t *ref, uint32_t flag, int device);

/* The same context over SEVERAL devices of one node (multi-GPU behind this ABI): reads shard
 * embarrassingly, so the context owns one ordinary context per entry of devices[] and every align call below cuts its
 * batch into contiguous read ranges [r*n/G, (r+1)*n/G), runs them side by side (one host thread per device inside the
 * call) and writes the rows into the caller's array in input order -- no collective on the data path.  The reference
 * event model crosses PCIe once, to devices[0], and travels device to device from there (hipMemcpyPeer, xGMI between the
 * GPUs of a node): the "broadcast, root 0" of the multi-GPU design.  A device may be listed more than once (two shards on
 * one GPU).  Works with sfa_align_batch, sfa_submit_batch / sfa_wait_batch, sfa_align_events, sfa_align_raw(_ex),
 * sfa_set_option (applies to every shard), sfa_sync, sfa_get_profile (slowest shard's times, summed counts), sfa_destroy;
 * sfa_align_batch_device and sfa_stream need a single-device context (device memory and streams belong to one GPU). */
int sfa_init_devices(sfa_ctx_t **ctx, const sfa_ref_t *ref, uint32_t flag, const int *devices, int n_devices);

/* Shards behind a context: 1 for sfa_init, n_devices for sfa_init_devices. */
int sfa_n_devices(sfa_ctx_t *ctx);

/* Align a batch.  queries: concatenated, already z-normalised event means in EVENT order (the library applies
 * the RNA reversal of src/sigfish.c:860-866 itself); q_off[n_reads+1] offsets into queries; a read with
 * q_off[i+1]==q_off[i] is skipped (valid=0).  out[n_reads] is written in input order.  Blocking. */
int sfa_align_batch(sfa_ctx_t *ctx, const float *queries, const int64_t *q_off, int32_t n_reads, sfa_result_t *out);

/* Same with queries and results resident in device memory (d_queries: floats in HBM, d_out: n_reads rows in
 * HBM); q_off stays a HOST array.  Work is enqueued on the context stream; returns after enqueueing unless
 * `sync` is non-zero. */
int sfa_align_batch_device(sfa_ctx_t *ctx, const float *d_queries, const int64_t *q_off, int32_t n_reads,
                           sfa_result_t *d_out, int sync);

/* The same call split in two, so that the host can load and event-detect batch i+1 while batch i is on the GPU
 * (the overlap the reference's strictly serial load -> process -> output loop, src/dtw_main.c:299-326, lacks).
 * sfa_submit_batch returns once the work is queued; `queries` must stay valid until sfa_wait_batch, which blocks,
 * fills out[n_reads] and must be called with the same n_reads.  One batch in flight per context: a second submit
 * waits for the first to finish and discards its rows (if that batch failed on the device, SFA_EKERNEL, the second
 * submit returns its error).  sfa_align_batch == submit + wait. */
int sfa_submit_batch(sfa_ctx_t *ctx, const float *queries, const int64_t *q_off, int32_t n_reads);
int sfa_wait_batch(sfa_ctx_t *ctx, sfa_result_t *out, int32_t n_reads);

/* Secondary mappings (option "secondary" = 1..4, see sfa_set_option): the candidates behind the primary in the reference's own
 * sorted list of the 5 best per read (aln[3], aln[2], aln[1], aln[0] of update_aln, src/sigfish.c:575-626; ties: the later
 * candidate ranks higher), of the most recently completed call (a synchronous call or sfa_wait_batch; call this before the next
 * batch is submitted).  sec[i*4+k], k = 0 the best secondary: rid, strand, pos_st/pos_end (flipped and offset as the primary),
 * score, score2 = the score of the next candidate below it (+inf for the last), mapq 0.  Slots beyond the option, slots whose
 * score is not finite, and -- unless the option "secondary_strips" is 1 -- every slot of a read of more than SFA_MAX_QUERY events
 * have valid = 0.  With "secondary_strips" the row strips keep such a read's list as well: its slots are filled by the same rule,
 * through every entry point, and sfa_event_maps takes its rows like any others.
 * No de-duplication: neighbouring windows of one locus often fill the list.  Returns SFA_EINVAL when the option is 0. */
int sfa_secondary_rows(sfa_ctx_t *ctx, sfa_result_t *sec, int32_t n_reads);

/* The reference-column -> query-event maps (aln_t.r2qevent_map, path_to_map, src/sigfish.c:530-571) of a whole batch of rows from
 * the device: what sfa_r2qevent_map computes per read on a host thread.  Refers to the most recently completed align call of the
 * context (sfa_align_batch, sfa_wait_batch, sfa_align_events, sfa_align_raw(_ex), sfa_align_blow5; call this before the next batch
 * is submitted, as for sfa_secondary_rows): its queries are still resident, nothing is uploaded again.  rows[n_rows]: rows that
 * call returned -- primaries, or rows of sfa_secondary_rows; read_of_row[k]: the read of row k in that call (NULL: the identity,
 * and n_rows must be its read count).  map_off[n_rows+1]: the caller's offsets into `pairs`, in pairs; the map of row k --
 * pos_end - pos_st + 1 pairs, layout exactly sfa_r2qevent_map's -- is written at pairs + 2 * map_off[k].  A smaller gap for a
 * valid row is SFA_ERANGE; rows with valid = 0 or rid < 0 write nothing, and neither does a row for which sfa_r2qevent_map would
 * return SFA_EINVAL.  The band of every row is filled again on the device with the arithmetic of the host routine (bit-identical
 * costs, same tie order) in slices whose packed moves fit "map_scratch_bytes"; a row whose own moves exceed that budget, or whose
 * read has more than SFA_MAX_QUERY events, is computed by the host routine inside the call -- *n_on_host (may be NULL) counts them.
 * With the option "map_strips" a read of more than SFA_MAX_QUERY events stays on the device: its band is filled in strips of
 * SFA_MAX_QUERY query rows, one launch per strip level, each strip starting from the bottom row of the one above; only a row
 * whose own moves exceed the budget then goes to the host routine and counts.  The maps are the same bytes either way.
 * SFA_EINVAL: no completed call, a read count or read index that does not match it, or the last call was
 * sfa_align_batch_device (its queries are the caller's).  Group contexts split the rows by the shard that holds their read. */
int sfa_event_maps(sfa_ctx_t *ctx, const sfa_result_t *rows, const int32_t *read_of_row, int32_t n_rows, const int64_t *map_off,
                   int32_t *pairs, int32_t *n_on_host);

/* ---- alignment sessions: a read's alignment extended as its events arrive (real-time use) -------------------------------
 * A session has n_slots SLOTS, each one growing read (a sequencing channel, say).  Of every (slot, contig, strand) sweep it keeps
 * the last query row in device memory -- the accumulated cost of every reference column and, unless SFA_SESSION_NO_START, the
 * start column of the path into it -- so a chunk of new events costs its own rows of the recurrence, however long the read has
 * become, instead of sfa_align_batch over the whole prefix again.  The caller keeps its normalisation fixed over a slot's life:
 * the events of all chunks are taken as ONE query (to re-normalise, reset the slot and send its events again).
 * Single-device contexts (or, with SFA_SESSION_SPREAD, the devices of sfa_init_devices) without SFA_DTW, and not SFA_RNA without SFA_INV (the query rows are then the events reversed: new events
 * would become row 0) unless the session is created with SFA_SESSION_RESWEEP; SFA_EINVAL otherwise.  A session belongs to its context and uses its stream; its buffers are its own, so
 * batch calls on the context between two extends do not disturb it, and sfa_secondary_rows / sfa_event_maps keep referring to
 * the last BATCH call.  sfa_destroy frees the sessions a context still has: their handles are dead after it. */
typedef struct sfa_session sfa_session_t;
#define SFA_SESSION_NO_START 0x1 /* carry costs only: half the memory, the fill's cheap cell; the start side is not reported */
/* 0x2 is not assigned: sfa_session_bytes and sfa_session_create refuse it as an unknown bit. */
#define SFA_SESSION_RESWEEP 0x4  /* raw mode only: a slot is swept when its normalisation window changes, over the window's events
                                    (see "resweep sessions" below); accepts SFA_RNA without SFA_INV */
/* 0x8 is not assigned either. */
#define SFA_SESSION_SPREAD 0x10  /* on a context of sfa_init_devices: the slots are dealt over its devices (see below) */
/* Spread sessions.  Without SFA_SESSION_SPREAD a session needs a single-device context.  With it, on a context of G shards
 * (sfa_init_devices), the session is one ordinary session per shard that holds slots, created with the caller's other flags:
 * slot i lives on shard i % G as that shard's slot i / G, so consecutive channels balance, and device r holds the bytes of
 * (n_slots - r + G - 1) / G slots -- carried rows (sfa_session_bytes), and the same share of everything the configuration calls
 * add.  With n_slots < G the trailing shards hold nothing.  If one shard cannot create its part (SFA_ENOMEM on one device), the
 * parts already made are freed and the call fails with that shard's code and message.  On a single-device context the flag is
 * accepted and changes nothing.
 * Every entry point below works on a spread session with the same arguments and the same results, byte for byte, as on a plain
 * session fed the same calls; slot numbers are always the caller's, and the forms without a slot list answer in slot order.  A
 * call's entries are dealt to the shards (the caller's order kept inside each), the shards run side by side on the context's
 * shard threads -- shard 0 on the caller's -- and the answers are put back in the caller's order.  The chunks of
 * sfa_session_extend and sfa_session_extend_raw are packed per shard into host buffers the session owns and reuses: a tick
 * allocates nothing once they have grown to its size.  sfa_session_event_maps writes every shard's maps straight into the caller's
 * pairs.  sfa_session_row and sfa_session_events go to the shard that owns the slot.
 * Refusals: a slot out of range or named twice is refused for the whole call before any shard hears of it, and so is whatever
 * else an extend call is refused for (a slot past its end of read, another scaling, ...): every shard is asked before any shard
 * works, so a refused call changes nothing on any shard.  An error a shard meets while it works is the call's error, the first in
 * shard order; the other shards have then done their part of the call.
 * Configuration (sfa_session_raw_config, sfa_session_raw_recalibrate, sfa_session_raw_auto_start, sfa_session_candidates_config,
 * sfa_session_keep_events) goes to every shard.  What it is refused for -- the arguments, the session's kind, a slot in use
 * anywhere -- is the same on every shard, and every shard refuses.  If one shard fails for a reason of its own (memory) after
 * another has taken the call, the call returns that error and the session takes nothing but sfa_session_destroy from then on
 * (SFA_EINVAL).
 * sfa_get_profile on the context afterwards reports the call as it reports a sharded batch: the slowest shard's times, the summed
 * counts; a shard the call had nothing for adds nothing.  sfa_destroy frees a context's spread sessions before its shards. */

/* SFA_ENOMEM when the carried rows do not fit. */
int sfa_session_create(sfa_ctx_t *ctx, int32_t n_slots, uint32_t session_flags, sfa_session_t **s);

/* Append events[ev_off[i] .. ev_off[i+1]) -- z-normalised means in event order, as for sfa_align_batch -- to slot slot[i], i < n,
 * and write to out[i] the row sfa_align_batch returns for ALL events the slot has received since its last reset: every field,
 * bit for bit.  With SFA_SESSION_NO_START the coordinate that needs the start column is -1 instead: pos_st on '+', pos_end on
 * '-' (the flip).  Chunks may have any length (one of more than SFA_MAX_QUERY events runs as consecutive pieces inside the
 * call); an empty chunk returns the slot's current row, valid = 0 for a slot without events.  A chunk with a NaN or +-inf
 * poisons its slot: its rows are valid = 0 until it is reset, and it counts in sfa_profile_t.non_finite_reads.  Blocking, on the
 * context's stream.  SFA_EINVAL: a slot out of range or named twice in the call.  sfa_get_profile afterwards reports this call:
 * fill_ms (the sweeps), total_ms, cells (new events x reference columns), n_tasks. */
int sfa_session_extend(sfa_session_t *s, const int32_t *slot, const float *events, const int64_t *ev_off, int32_t n,
                       sfa_result_t *out);

/* Forget the events of slot[0..n) (slot == NULL: of every slot); a poisoned slot is clean again. */
int sfa_session_reset(sfa_session_t *s, const int32_t *slot, int32_t n);

/* len[i] = events slot[i] has received since its last reset (slot == NULL: all slots in order, n must be n_slots). */
int sfa_session_lengths(sfa_session_t *s, const int32_t *slot, int32_t n, int64_t *len);

/* The carried row of (slot, contig, strand_char '+' or '-') read back: cost[j] = accumulated cost of the last query row at column
 * j of that strand's array, start[j] (start may be NULL) = the column in which the path into that cell begins.  Both are given as
 * stored: columns of the strand's OWN array, before the flip of '-' and before ref_st_offset that the rows of sfa_session_extend
 * have applied.  Returns the number of columns (the contig's ref_length); the caller's arrays hold at least that many.  A
 * device-to-host copy on the context's stream, blocking; for checking and debugging, not for the hot path.  SFA_EINVAL: a slot,
 * contig or strand that does not exist (SFA_RNA has no '-'), start != NULL on a SFA_SESSION_NO_START session, a slot without
 * events, a poisoned slot. */
int64_t sfa_session_row(sfa_session_t *s, int32_t slot, int32_t contig, int32_t strand_char, float *cost, int32_t *start);

/* Session candidates: the secondary mappings of the real-time path.  With n_candidates = 1..4 a session keeps, behind every
 * slot's row, the next n_candidates entries of the reference's sorted list of the 5 best windows (update_aln, src/sigfish.c:575-626;
 * ties: the later candidate ranks higher) over ALL events the slot has received: what sfa_secondary_rows returns for a batch.  The
 * sweep keeps each window's first strict minimum with its start column in a list per (slot, contig, strand), and a merge over the
 * jobs in processing order writes the rows: no second pass, and, unlike sfa_secondary_rows, NO SFA_MAX_QUERY cut-off -- a slot with
 * more than SFA_MAX_QUERY events has valid candidates.  n_candidates = 0 switches the lists off: the session launches the kernels
 * it launched before.  Rows, carried rows and everything else a session returns are the same bytes with and without.  Allowed only
 * while every slot is empty, as for sfa_session_raw_config (SFA_EINVAL otherwise, and for n_candidates outside 0..4); works on
 * event-mode, raw-mode and resweep sessions, with or without SFA_SESSION_NO_START.  It is no session flag. */
int sfa_session_candidates_config(sfa_session_t *s, int32_t n_candidates);

/* sec[i*4+k], k = 0 the best: the candidates behind the row slot[i] currently has -- the row sfa_session_extend /
 * sfa_session_extend_raw last returned for it, or would return for an empty chunk (on a resweep session: of the window the row
 * spans).  Layout exactly as sfa_secondary_rows: rid, strand, pos_st / pos_end flipped and offset as the primary (with
 * SFA_SESSION_NO_START the coordinate that needs the start column is -1, as in the primary), score, score2 = the score of the
 * next candidate below (+inf for the last), mapq 0; valid = 0 for ranks beyond n_candidates and for entries that are empty or not
 * finite (a slot with fewer windows than ranks).  Where sec[i*4] is valid its score is the primary's score2.  A slot without events
 * and a poisoned slot give four rows with valid = 0.  No de-duplication: neighbouring windows of one locus often fill the list --
 * which is what a caller looks at to tell a depressed mapq from a second locus.  Blocking, on the context's stream.  SFA_EINVAL:
 * the session keeps no candidates, a slot out of range. */
int sfa_session_candidates(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_result_t *sec);

void sfa_session_destroy(sfa_session_t *s);

/* Device memory sfa_session_create takes for the carried rows of n_slots slots over a reference of total_columns columns
 * (sum of ref_lengths, twice that for DNA): one row per slot, updated in place -- total_columns x n_slots x 8 bytes, x 4 with
 * SFA_SESSION_NO_START (the allocator adds an eighth of headroom; bookkeeping is some 50 bytes per slot, and 96 more -- four rows -- on a
 * session that keeps candidates, sfa_session_candidates_config: not counted here).  Host arithmetic, no
 * device needed; negative (an SFA_E* code) for arguments that are not positive, unknown flags or a product beyond 2^63.
 * SFA_SESSION_RESWEEP changes nothing: the carried rows are still needed (a window beyond SFA_MAX_QUERY events runs as pieces).
 * Neither does SFA_SESSION_SPREAD: the session holds the same rows, device r of G those of (n_slots - r + G - 1) / G slots. */
int64_t sfa_session_bytes(int64_t total_columns, int32_t n_slots, uint32_t session_flags);

/* ---- target classes: the best on-target and the best off-target score of a slot ----------------------------------------------
 * Adaptive sampling asks whether a read comes from a region the user wants, not where exactly it maps.  The mapq of a row is
 * built from the two best windows anywhere, so two good windows inside one target depress it, and a read with nothing good on
 * target never reaches it.  What answers the question is the lowest cost among the carried row's on-target columns against the
 * lowest among the others -- data the session holds already (the rows sfa_session_row copies back).
 * A target is an interval [begin, end) of one contig in the coordinates a row reports (sfa_result_t.pos_st / pos_end: after
 * the strand flip and ref_st_offset).  Column j of job (contig, strand) is ON target when the coordinate a row reports for an
 * alignment that ENDS in column j lies in an interval of that contig: j + ref_st_offset on '+' (the row's pos_end) and
 * ref_length - j + ref_st_offset on '-' (there the end column is the row's pos_st; its pos_end needs the start column, which a
 * SFA_SESSION_NO_START session does not carry).  Intervals may overlap, touch and come in any order.
 * The mask is one bit per column of a slot's row -- total_columns / 8 bytes per SESSION, shared by all slots, not counted by
 * sfa_session_bytes; a call adds 16 bytes per named slot and 8192 columns, and 40 bytes per named slot. */
typedef struct {
    int32_t contig, begin, end;
} sfa_target_t;

/* A slot's class result: cost, contig, coordinate (as above) and strand of the best on-target and the best off-target column.
 * Ties: the lowest cost, then the lowest column of the slot's row -- jobs in their order, '+' before '-', then the lowest column
 * of the job.  A class without columns: score +inf, rid -1, pos_end -1, strand 0.  n_events: events the slot has received;
 * valid 0: the slot is empty or poisoned (scores +inf, rids -1). */
typedef struct {
    float on_score, off_score;
    /* on_pos_end / off_pos_end: the END-COLUMN coordinate of the class's best column -- where an alignment ending in that column
     * ends in the coordinates rows report.  On '+' that is the pos_end a finalized row reports; on '-' the flip makes it the
     * row's pos_st (the row's pos_end there is built from the START column, which a class does not know). */
    int32_t on_rid, on_pos_end, off_rid, off_pos_end;
    int8_t on_strand, off_strand;
    int8_t pad[2];
    int32_t n_events;
    int32_t valid;
} sfa_class_t;

/* Sets the session's targets: the mask is built on the host and uploaded.  n = 0 switches the feature off and frees the mask.
 * Allowed at any time (the mask does not depend on the slots' state).  On a spread session it goes to every sub-session.
 * SFA_EINVAL: a contig out of range, begin < 0, end <= begin, end beyond the contig (the largest coordinate a row of the contig
 * reports is ref_st_offset + ref_length, so end may be one more); a SFA_SESSION_RESWEEP session (its carried row belongs to the
 * reversed query; what its minimum means has not been looked into).  SFA_ERANGE: a reference of 2^31 columns or more. */
int sfa_session_targets(sfa_session_t *s, const sfa_target_t *targets, int32_t n);

/* Columns of a slot's row that are on target (0 without targets; on a spread session every sub-session holds the same mask). */
int64_t sfa_session_target_columns(sfa_session_t *s);

/* The class results of slot[0..n) into out[0..n).  One masked min-reduction over the slots' carried cost rows (no sweep kernel
 * changes, a session without targets launches what it always launched), event mode and raw mode, with and without
 * SFA_SESSION_NO_START.  Blocking, on the context's stream; sfa_profile_t.class_ms is its device time (the other fields of the
 * profile are zero).  A spread session partitions the call by shard and answers in the caller's order.
 * SFA_EINVAL: no targets, a slot out of range or named twice. */
int sfa_session_classes(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_class_t *out);

/* The decision from a class result (host only): with n = n_events >= min_events, off_score - on_score >= margin * n says ON
 * target, on_score - off_score >= margin * n says OFF target; an empty class counts as +inf, both empty decide nothing.
 * mode 0 (enrich): on -> 'A' (accept), off -> 'U' (unblock); mode 1 (deplete): the other way round.  0: no decision (also for
 * valid = 0, an unknown mode, a margin that is negative or not finite).  Queries are z-normalised, so a per-event margin has no
 * unit.  Nobody has measured a good margin: there is no default. */
int sfa_target_decide(const sfa_class_t *cls, int32_t mode, int32_t min_events, float margin);

/* ---- coverage caps: targets that close where they are covered deeply enough ------------------------------------------------------
 * The session keeps a depth track per contig on the device: one uint32 per coordinate a row of the contig can report, ref_length + 1
 * entries, entry x - ref_st_offset for coordinate x, both strands sharing it (depth belongs to the position).  The LIVE mask is
 * derived from the mask of sfa_session_targets (the base mask, which is kept) and the tracks: a column is live when its bit of the
 * base mask is set and the depth of the coordinate the column reports (as for the mask above) lies below the cap.  While a cap is
 * set, sfa_session_classes reads the live mask -- a closed coordinate is OFF target on both strands -- and
 * sfa_session_target_columns reports the live columns.  Memory: 4 bytes per coordinate and a second mask per SESSION
 * (sfa_session_coverage_bytes), not counted by sfa_session_bytes; a session that never sets a cap allocates nothing and launches
 * what it launched before.  Depth does not saturate: with caps of at most 2^30 and at most 2^20 intervals a call, a coordinate
 * wraps only after 2^32 additions, 4096 calls that each cover it 2^20 times -- no run of the front ends, which add at most one
 * interval per accepted read, comes near.
 * On a spread session _config and _add go to every sub-session (every shard holds the same mask and tracks); _depth is answered
 * by shard 0, and open_columns is shard 0's count, not a sum. */

/* cap >= 1 switches the feature on (depth zeroed, live mask = base mask); cap = 0 switches it off and frees both buffers.
 * Needs targets (sfa_session_targets); allowed at any time, as the mask does not depend on the slots.  sfa_session_targets on a
 * session with a cap rebuilds the base mask and derives the live mask from the kept depth; with n = 0 it drops the cap too.
 * SFA_EINVAL: a null session, cap < 0 or cap > 2^30, no targets. */
int sfa_session_coverage_config(sfa_session_t *s, int32_t cap);
/* depth += 1 over every interval (sfa_target_t: contig, [begin, end) in the coordinates rows report; the part of an interval
 * below ref_st_offset, which no row reports, counts nowhere), then the live mask is derived again; *open_columns (may be NULL)
 * receives the live on-target columns.  Intervals may overlap each other; n = 0 adds nothing and derives the mask.  One call,
 * blocking, on the context's stream; sfa_profile_t.class_ms is its device time.
 * SFA_EINVAL, before anything is written: null arguments, no cap set, more than 2^20 intervals, an interval sfa_session_targets
 * would refuse as a target (same messages). */
int sfa_session_coverage_add(sfa_session_t *s, const sfa_target_t *iv, int32_t n, int64_t *open_columns);
/* a contig's track back: out[0 .. ref_length + 1).  SFA_EINVAL: null arguments, no cap set, a contig out of range, n other than
 * ref_length + 1. */
int sfa_session_coverage_depth(sfa_session_t *s, int32_t contig, uint32_t *out, int32_t n);
/* Device memory a cap adds to a session of a context made from (ref, flag): 4 bytes per coordinate and the second mask.  Host
 * arithmetic; 0 for a null or empty reference. */
size_t sfa_session_coverage_bytes(const sfa_ref_t *ref, int flag);

/* ---- target groups: the best score per named group of targets (WHICH target a read hits) --------------------------------------
 * A group target is a target with a group id in [0, n_groups), 1 <= n_groups <= 1023.  Every column of a slot's row carries one
 * label: the lowest group id among the intervals that cover it (covered as for the mask above: the coordinate of an alignment
 * ENDING in the column), or n_groups -- the background -- when none does.  A group may have no column.  The label table is one
 * uint16 per column, 2 * total_columns bytes per SESSION, shared by all slots, not counted by sfa_session_bytes; a call adds
 * 8 * (n_groups + 1) bytes of keys and 16 * (n_groups + 1) + 24 bytes of results per named slot.  A session may hold a mask and
 * a label table side by side; neither knows of the other. */
typedef struct {
    int32_t contig, begin, end, group;
} sfa_group_target_t;

/* The best column of one entry (a group, or the background at index n_groups) of a slot: cost, contig, END-COLUMN coordinate
 * and strand as in sfa_class_t; ties as there.  An entry without columns: +inf, -1, -1, 0. */
typedef struct {
    float score;
    int32_t rid, pos_end;
    int8_t strand;
    int8_t pad[3];
} sfa_group_best_t;

/* The two best entries of a slot, indices into [0, n_groups]; -1: no such entry (no entry has a column / only one has).  Equal
 * scores: the entry holding the lower column is `best`.  valid 0: the slot is empty or poisoned (-1, -1, +inf, +inf). */
typedef struct {
    int32_t best, second;
    float best_score, second_score;
    int32_t n_events, valid;
} sfa_group_head_t;

/* Sets the session's group targets; n = 0 switches the feature off and frees the table.  Allowed at any time; refusals as for
 * sfa_session_targets (a SFA_SESSION_RESWEEP session included), and SFA_EINVAL for n_groups outside 1 .. 1023 or a group id
 * outside [0, n_groups).  On a spread session it goes to every sub-session. */
int sfa_session_target_groups(sfa_session_t *s, const sfa_group_target_t *targets, int32_t n, int32_t n_groups);

/* n_groups of the session, 0 without groups. */
int32_t sfa_session_group_count(sfa_session_t *s);

/* The group results of slot[0..n): bests[n][n_groups + 1] (may be NULL) and heads[n].  One labelled min-reduction over the
 * slots' carried cost rows; event mode and raw mode, with and without SFA_SESSION_NO_START.  Blocking, on the context's stream;
 * sfa_profile_t.class_ms is its device time.  A spread session partitions the call by shard and answers in the caller's order.
 * SFA_EINVAL: no groups, a slot out of range or named twice. */
int sfa_session_group_bests(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_group_best_t *bests, sfa_group_head_t *heads);

/* The decision from a head (host only): the index of the best entry (a group, or n_groups for the background) when
 * n_events >= min_events and second_score - best_score >= margin * n_events, an empty runner-up (second < 0) counting as +inf;
 * otherwise -1 -- also for valid = 0, no best entry, a margin that is negative or not finite.  No default margin, as above. */
int sfa_group_decide(const sfa_group_head_t *h, int32_t min_events, float margin);

/* ---- open and closed groups: the class decision over groups that are still wanted (quotas) -------------------------------------
 * A bitmap of open groups comes with every call: (n_groups + 31) / 32 words of 32 bits, bit g % 32 of word g / 32 set: group g
 * is open -- still wanted.  Bits at or above n_groups are ignored; a NULL bitmap says every group is open.  A column is ON when
 * its label (above: the lowest group id that covers it) is a group and that group's bit is set; every other column is OFF -- the
 * background and every closed group.  Closing a group is clearing a bit on the host: no mask is rebuilt, nothing is uploaded.
 * cls is filled exactly as sfa_session_classes fills it for the mask of the open groups' columns (ties, empty classes and classes
 * of +inf columns as there), so sfa_target_decide applies unchanged.  on_group: the label of the best ON column; off_group: the
 * label of the best OFF column, a closed group's id or n_groups for the background; -1: the class has no column.
 * valid 0 (an empty or poisoned slot): scores +inf, rids, coordinates and groups -1. */
typedef struct {
    sfa_class_t cls;
    int32_t on_group, off_group;
} sfa_open_class_t;

/* The open-class results of slot[0..n) into out[0..n) under `open` (n_words words, or NULL).  One two-class min-reduction over
 * the slots' carried cost rows whose classes come from the session's label table (sfa_session_target_groups) and the bitmap; no
 * mask (sfa_session_targets) is needed, a session may hold one anyway.  Event mode and raw mode, with and without
 * SFA_SESSION_NO_START.  Blocking, on the context's stream; sfa_profile_t.class_ms is its device time.  A spread session
 * partitions the call by shard, every shard gets the bitmap, and answers come in the caller's order.  A call adds 16 bytes per
 * named slot and 8192 columns and 48 bytes per named slot of session scratch; once per label table the host finds the lowest
 * column of every label (4 * (n_groups + 1) bytes).  A session that never calls it launches what it launched before.
 * SFA_EINVAL (before anything is written to out): no groups, a slot out of range or named twice, `open` given with n_words other
 * than (n_groups + 31) / 32. */
int sfa_session_open_classes(sfa_session_t *s, const int32_t *slot, int32_t n, const uint32_t *open, int32_t n_words, sfa_open_class_t *out);

/* ---- group caps: named groups that close, column by column, where they are covered deeply enough -------------------------------
 * The LIVE label table is derived from the label table of sfa_session_target_groups (the base table, which is kept) and the depth
 * tracks of the coverage caps above: the live label of a column is its base label while the depth of the coordinate the column
 * reports lies below the group cap, and the background, n_groups, from then on.  A background column stays background; a column
 * two groups cover goes to the background with its coordinate, not to the higher group.  While a group cap is set,
 * sfa_session_open_classes and sfa_session_group_bests read the live table (the same kernels, another pointer): a group whose
 * every column is capped has no column, as a group without intervals has none.
 * A session has ONE depth track, shared by the mask's cap (sfa_session_coverage_config) and the group cap, which are two numbers:
 * whichever is configured first allocates the track, zeroed; it is freed when both are 0.  Configuring either cap again zeroes the
 * track only while the other cap is off.  sfa_session_coverage_config(s, 0) and sfa_session_targets(s, NULL, 0) keep the track
 * while a group cap is on; on a session that never sets a group cap every call above does what it did.  With either cap set
 * sfa_session_coverage_add adds once to the track and derives, in the same call, whichever of the live mask and the live labels
 * are on (open_columns: sfa_session_target_columns' answer), and sfa_session_coverage_depth answers.
 * Memory: sfa_session_group_coverage_bytes per SESSION, not counted by sfa_session_bytes.
 * On a spread session _config goes to every sub-session and sfa_session_group_coverage is answered by shard 0. */

/* The depth of one entry (a group, or the background at index n_groups), taken over the columns of the FORWARD ('+') jobs whose
 * BASE label is the entry: every coordinate a forward row reports counts once; the one coordinate per contig that only a reverse
 * row reports (ref_st_offset + ref_length) is left out.  capped: columns whose depth is at or above the group cap.  An entry
 * without columns: 0, 0, 0, UINT32_MAX, 0 -- form no mean from it. */
typedef struct {
    int64_t columns, capped;
    uint64_t depth_sum;
    uint32_t depth_min, depth_max;
} sfa_group_cover_t;

/* cap >= 1 switches the group cap on (live table = base table where the kept depth allows); cap = 0 switches it off and frees the
 * live table.  Needs groups (sfa_session_target_groups), no mask.  sfa_session_target_groups on a session with a group cap rebuilds
 * the base table and derives the live one from the kept depth; with n = 0 it drops the group cap too.
 * SFA_EINVAL: a null session, cap < 0 or cap > 2^30, no groups (so every SFA_SESSION_RESWEEP session). */
int sfa_session_group_coverage_config(sfa_session_t *s, int32_t cap);
/* The records of the n_groups + 1 entries into out[0 .. n).  Blocking, on the context's stream; sfa_profile_t.class_ms is its
 * device time.  SFA_EINVAL, before anything is written: null arguments, no group cap set, n other than n_groups + 1. */
int sfa_session_group_coverage(sfa_session_t *s, sfa_group_cover_t *out, int32_t n);
/* Device memory a group cap takes on a session of a context made from (ref, flag) with n_groups groups: the depth tracks (4 bytes
 * per coordinate; shared with the mask's cap, so not taken twice), the second label table (2 bytes per column) and 36 bytes per
 * entry.  Host arithmetic; 0 for a null or empty reference or n_groups outside 1 .. 1023. */
size_t sfa_session_group_coverage_bytes(const sfa_ref_t *ref, int flag, int32_t n_groups);

/* ---- reach targets: stranded targets with a lead-in (will the read REACH a target?) ------------------------------------------------
 * A plain target (sfa_target_t) asks where a read's alignment ends NOW.  A decision is taken after a few hundred events on a read
 * that runs on for kilobases, and in a direction: on '+' towards higher coordinates, on '-' towards lower ones.  A reach target
 * is a target with a strand and a lead, the bases in front of it -- in the read's direction -- that count as on target.
 * With x the coordinate column j of job (contig c, strand s) reports (as for the mask above), target t ADMITS the column when
 * t.contig == c, t.strand is 0 or s, and
 *     on '+':  t.begin - t.lead <= x < t.end          on '-':  t.begin <= x < t.end + t.lead
 * (64-bit bounds; only the coordinates a row reports clip them).  A column is ON target when some target admits it.  Its ANCHOR
 * is the first base of a target the read will reach: on '+' the minimum over the admitting targets of max(x, t.begin), on '-' the
 * maximum of min(x, t.end - 1).  With every lead 0 and every strand 0 the mask is sfa_session_targets' and the anchor is x.  On a
 * context without '-' jobs (SFA_RNA) a '-' target admits nothing; that is allowed.
 * Under a depth cap (sfa_session_coverage_config) a column of a reach session is live while its bit of the base mask is set and
 * the depth of its ANCHOR lies below the cap: a lead-in closes when the bases it leads to are covered, not when it is itself.
 * The mask and the anchors are built on the device from a sorted form of the list prepared on the host.  Memory: the mask of
 * sfa_session_targets and 4 bytes per column per SESSION (sfa_session_reach_bytes), not counted by sfa_session_bytes; a session
 * that never calls sfa_session_targets_reach allocates nothing and launches what it launched before.
 * Target groups (sfa_session_target_groups, open classes, group caps) work from labels; a label table with reach is set by
 * sfa_session_target_groups_reach below.  The mask's anchors and a label table's are two tables: neither knows of the other. */
typedef struct {
    int32_t contig, begin, end; /* [begin, end) in the coordinates rows report, as sfa_target_t */
    int32_t lead;               /* bases in front of the target, in the read's direction, that count as on target */
    int8_t strand;              /* '+', '-', or 0: both */
    int8_t pad[3];              /* zero */
} sfa_reach_target_t;

/* Sets the session's targets from a reach list; it replaces whatever mask the session held, as a later sfa_session_targets
 * replaces it in turn (and frees the anchors).  n = 0 switches targets off, as sfa_session_targets(s, NULL, 0) does.  Allowed at
 * any time; the depth track of a cap is kept across either change and the live mask is derived again.  sfa_session_classes,
 * sfa_session_target_columns and sfa_session_coverage_config / _add / _depth read whichever mask is current.  On a spread session
 * it goes to every sub-session.
 * SFA_EINVAL, before anything is written: everything sfa_session_targets refuses (same messages, a SFA_SESSION_RESWEEP session
 * included), lead < 0 or lead > 2^30, a strand other than 0, '+', '-', padding that is not zero, more than 2^20 targets.
 * An allocation or device failure AFTER the list has passed (SFA_ENOMEM, SFA_ENODEV, SFA_EKERNEL) leaves the session without
 * targets, as sfa_session_targets(s, NULL, 0) does -- a mask cap goes with them, and its depth track unless a group cap holds it.
 * During the call the prepared runs take 16 bytes each on the device (about three per target and strand); they are freed before
 * it returns. */
int sfa_session_targets_reach(sfa_session_t *s, const sfa_reach_target_t *targets, int32_t n);
/* The base mask (n_words: total_columns / 32 rounded up, and one more word, which is zero; bit j & 31 of word j >> 5 is column
 * j) and the anchors (n_cols: total_columns; the anchor of column j as an index into its contig's depth track -- coordinate -
 * ref_st_offset -- or -1: the column is off target, or -2: the anchor lies below ref_st_offset, where no row reports and no
 * depth is counted) back from the device.  Either pointer may be NULL.  On a spread session shard 0 answers.
 * SFA_EINVAL: no reach targets, n_words or n_cols other than the above. */
int sfa_session_reach_tables(sfa_session_t *s, uint32_t *mask, size_t n_words, int32_t *anchor, int64_t n_cols);
/* Device memory the anchors take on a session of a context made from (ref, flag): 4 bytes per column.  Host arithmetic; 0 for a
 * null or empty reference. */
size_t sfa_session_reach_bytes(const sfa_ref_t *ref, int flag);

/* ---- reach groups: named target groups with a lead-in (WHICH target will the read reach?) -------------------------------------
 * A reach group target is a reach target with a group id in [0, n_groups), 1 <= n_groups <= 1023.  Admission and the ANCHOR of a
 * column are those of the reach targets above, with the groups dropped: groups do not enter them.  The LABEL of a column is the
 * lowest group id among the admitting targets whose own anchor (max(x, t.begin) on '+', min(x, t.end - 1) on '-') equals the
 * column's anchor -- the target the read reaches first, ties to the lowest id -- or n_groups, the background, when nobody admits
 * the column.  With every lead 0 and every strand 0 the table is sfa_session_target_groups' bit for bit; inside a target's body
 * another group's lead-in never takes the label.
 * The label table replaces the session's label table; its anchors (one int32 per column, an index into the contig's depth track,
 * -1: background, -2: below ref_st_offset) are the label table's own and independent of a mask's.  sfa_session_group_bests,
 * sfa_session_open_classes and sfa_session_group_count work unchanged on it.  Under a group cap
 * (sfa_session_group_coverage_config) the live label of a column is its base label while the depth of its ANCHOR lies below the
 * cap (-2: depth 0): a lead-in closes when the base it leads to is covered, not when it is itself.  sfa_session_group_coverage
 * on a reach label table counts the forward jobs' BODY columns only, by base label -- a body column is one whose anchor is its
 * own coordinate; a lead-in column is part of no record, so a group that has only '-' targets has an empty record, and so has the
 * background.
 * Both tables are built on the device from a sorted form of the list prepared on the host.  Memory: 2 + 4 bytes per column per
 * SESSION (sfa_session_group_reach_bytes), not counted by sfa_session_bytes; a session that never calls
 * sfa_session_target_groups_reach allocates nothing new and launches what it launched before. */
typedef struct {
    int32_t contig, begin, end; /* [begin, end) in the coordinates rows report, as sfa_target_t */
    int32_t lead;               /* bases in front of the target, in the read's direction, that carry its label */
    int32_t group;              /* 0 .. n_groups - 1 */
    int8_t strand;              /* '+', '-', or 0: both */
    int8_t pad[3];              /* zero */
} sfa_reach_group_target_t;

/* Sets the session's label table from a reach group list; it replaces whatever label table the session held, as a later
 * sfa_session_target_groups replaces it in turn (and frees the group anchors).  n = 0 switches groups off, as
 * sfa_session_target_groups(s, NULL, 0, 0) does.  Allowed at any time; the depth track of a group cap is kept and the live table
 * is derived again.  On a spread session it goes to every sub-session.
 * SFA_EINVAL, before anything is written: everything sfa_session_targets_reach refuses (same messages, a SFA_SESSION_RESWEEP
 * session included), n_groups outside 1 .. 1023, a group id outside [0, n_groups).
 * An allocation or device failure AFTER the list has passed leaves the session without groups, as
 * sfa_session_target_groups(s, NULL, 0, 0) does -- a group cap goes with them.  During the call the prepared runs take 20 bytes
 * each on the device; they are freed before it returns. */
int sfa_session_target_groups_reach(sfa_session_t *s, const sfa_reach_group_target_t *targets, int32_t n, int32_t n_groups);
/* The BASE label table (n_cols: total_columns; one uint16 per column) and its anchors (n_cols int32, as above) back from the
 * device.  Either pointer may be NULL.  On a spread session shard 0 answers.
 * SFA_EINVAL: no reach groups, n_cols other than total_columns. */
int sfa_session_group_reach_tables(sfa_session_t *s, uint16_t *label, int32_t *anchor, int64_t n_cols);
/* Device memory the two tables take on a session of a context made from (ref, flag): 2 + 4 bytes per column.  Host arithmetic;
 * 0 for a null or empty reference. */
size_t sfa_session_group_reach_bytes(const sfa_ref_t *ref, int flag);

/* ---- truth: a target decision against where a read really came from (host only; no context, no device) --------------------------
 * A read's truth is the interval [begin, end) of `contig` its bases cover on the forward strand; contig < 0: the read belongs
 * nowhere.  These are the rules `sigfish-amd realtime --truth` applies (sigfish_amd/csrc/truth_rules.hpp), exported so that no
 * caller restates them.
 * sfa_truth_class: 'T' when the interval shares at least one base with a target of its contig, else 'O' (also for contig < 0).
 * An overlap rule on purpose: a class decision reads the alignment's END coordinate, so a read that straddles a target's edge may
 * honestly be decided either way; sfa_truth_edge is 1 for such a read -- overlapping, but contained in no single target -- else 0.
 * sfa_truth_group: the lowest group id among the overlapping group targets (the tie rule of a column's label), else n_groups,
 * the background.
 * sfa_truth_verdict: 'C' when the decided class equals the true one, 'W' when it differs, 'N' when either is no class (anything
 * but 'T' and 'O').  sfa_truth_group_verdict: the same over two entries (a group id, or n_groups for the background); a negative
 * entry is none, 'N'. */
int sfa_truth_class(const sfa_target_t *targets, int32_t n, int32_t contig, int32_t begin, int32_t end);
int sfa_truth_edge(const sfa_target_t *targets, int32_t n, int32_t contig, int32_t begin, int32_t end);
int32_t sfa_truth_group(const sfa_group_target_t *targets, int32_t n, int32_t n_groups, int32_t contig, int32_t begin, int32_t end);
int sfa_truth_verdict(int decided, int truth);
int sfa_truth_group_verdict(int32_t decided, int32_t truth);

/* ---- event maps of a slot's row: the warp path of the real-time path -------------------------------------------------------
 * sfa_session_event_maps is sfa_event_maps for rows a SESSION returned: the reference-column -> query-event map
 * (aln_t.r2qevent_map, the ss string of a SAM record) of every row, from the device, with nothing uploaded again.  rows[k] is a
 * row the session returned for slot slot_of_row[k] in the slot's CURRENT state: the primary of its last sfa_session_extend /
 * sfa_session_extend_raw (or of an empty chunk), or one of the four rows of sfa_session_candidates; one slot may be named any
 * number of times in a call.  map_off, pairs, the layout of a map (pos_end - pos_st + 1 pairs) and *n_on_host are exactly
 * sfa_event_maps's: rows with valid = 0 or rid < 0 write nothing (the rows of an empty or poisoned slot are such rows), a row for
 * which sfa_r2qevent_map returns SFA_EINVAL is left unwritten, a gap too small for a valid row is SFA_ERANGE.
 * The query of row k is the slot's query as swept, events [0, q_events): in raw mode the slot's normalised query where it lies in
 * device memory (on a resweep session the W events of the window as stored -- already reversed for SFA_RNA without SFA_INV); in
 * event mode the events the session kept (sfa_session_keep_events).  The band comes from the row, the flip and offset undone as
 * for sfa_event_maps; the same fill and walk kernels run it, in slices that follow "map_scratch_bytes".  A slot with more than
 * SFA_MAX_QUERY query events, or a row whose own moves exceed the budget, takes the host routine inside the call (that slot's
 * query is copied back) and counts in *n_on_host; with the context's option "map_strips" a slot beyond SFA_MAX_QUERY events runs
 * on the device in row strips, as for sfa_event_maps, and only a row beyond the budget is the host's.
 * Blocking, on the context's stream.  The scratch is the session's own: sfa_event_maps keeps referring to the last BATCH call and
 * returns the same bytes whether or not a session call came in between, and the reverse.
 * SFA_EINVAL: a SFA_SESSION_NO_START session (no start column, no band); an event-mode session that keeps no events, or a slot
 * that has outgrown max_events; a slot out of range; a valid row for a slot that is empty or poisoned; a row whose contig or
 * strand does not exist or whose band leaves its array. */
int sfa_session_event_maps(sfa_session_t *s, const sfa_result_t *rows, const int32_t *slot_of_row, int32_t n_rows,
                           const int64_t *map_off, int32_t *pairs, int32_t *n_on_host);

/* An event-mode session does not keep the caller's events.  With max_events > 0 every sfa_session_extend call also appends its
 * chunks to a per-slot copy in device memory (one more kernel in front of the sweep, no further copy or wait), the query
 * sfa_session_event_maps reads.  A slot that receives more than max_events events keeps sweeping and returning rows as before;
 * only its maps are refused (SFA_EINVAL) until it is reset.  0 switches it off: the session launches the kernels it launched
 * before.  Allowed while every slot is empty; SFA_EINVAL otherwise, and on a raw-mode or resweep session, whose query is kept
 * already (sfa_session_raw_config switches it off).  It is no session flag. */
int sfa_session_keep_events(sfa_session_t *s, int32_t max_events);

/* Device memory sfa_session_keep_events takes: n_slots x max_events x 4 bytes (one flag byte per slot counts as bookkeeping).
 * Host arithmetic; negative (an SFA_E* code) for arguments that are not positive or a product beyond 2^63. */
int64_t sfa_session_keep_bytes(int32_t n_slots, int32_t max_events);

/* ---- raw-signal sessions: a slot's samples in, its row out ----------------------------------------------------------------
 * A real-time caller has raw ADC samples per channel, a few hundred to a few thousand at a time, not normalised events.  In raw
 * mode a session runs the stages in front of the sweep on the device as well, and carries their state per slot:
 *   events         the streaming detector of sfa_event_stream_* (same arithmetic, same events, bit for bit), its state, the slot's
 *                  table of final events (means in pA) in device memory; detector parameters follow the context's SFA_RNA
 *   normalisation  final events 0 .. skip_events - 1 are dropped (the -p of the batch path).  Once final event skip + norm - 1
 *                  exists, mean and sd over the pA means of events [skip, skip + norm) are computed exactly as sfa_znormalise
 *                  does (two sequential fp32 loops, sqrt in double) and FROZEN until the slot is reset (unless
 *                  sfa_session_raw_recalibrate lets the window grow); event e >= skip enters the slot's query as
 *                  (mean_e - mean) / sd in fp32
 *   sweep          the new query events are handed to the session sweep straight from device memory; only the per-slot counts
 *                  cross PCIe in between (the planner of the sweep is host code)
 * At query_events query events (skip + query final events) the slot is FULL: its detector stops, later samples are only counted.
 * A frozen sd that is zero or not finite, or a query event that is not finite, POISONS the slot as a non-finite chunk does in
 * sfa_session_extend: rows valid = 0 until it is reset.
 * sfa_session_raw_config switches a session to raw mode (or changes the three sizes); allowed only while every slot is empty,
 * needs skip >= 0 and 25 <= norm <= query, SFA_EINVAL otherwise.  sfa_session_extend on a raw-mode session is SFA_EINVAL, and so
 * is sfa_session_extend_raw on a session that is not.  sfa_session_reset clears a slot's detector, events, normalisation and
 * scaling too; sfa_session_lengths reports the query events swept.
 *
 * Resweep sessions (SFA_SESSION_RESWEEP).  With SFA_RNA and without SFA_INV the query rows are the events REVERSED
 * (src/sigfish.c:860-863): a new event becomes row 0, every cell below it changes, and no carried row can be extended.  Such a
 * query can only be swept again, and a resweep session does that at the points where the normalisation changes anyway:
 *   - the window W of a slot is the rule of sfa_session_raw_recalibrate below, unchanged (frozen at norm without a list;
 *     SFA_RECAL_AT_END included);
 *   - when a call leaves the slot with another W than its row spans -- the first calibration is the case "from 0" -- the device
 *     computes mean and sd over final events [skip, skip + W), writes the query of W events,
 *     q[i] = z(event[skip + W - 1 - i]) for SFA_RNA without SFA_INV and q[i] = z(event[skip + i]) otherwise, and sweeps it as a
 *     first chunk inside that call (beyond SFA_MAX_QUERY events as consecutive pieces); a call that passes several points takes
 *     the last;
 *   - a call that does not change W sweeps nothing: out[i] is the slot's current row, and events beyond skip + W wait in the
 *     event table for the next point.
 * So after ANY call out[i] is, bit for bit, the row sfa_align_batch gives on the same context for the pA means of events
 * [skip, skip + W), z-normalised over themselves and given in event order (SFA_SESSION_NO_START as documented); info.q_events,
 * info.norm_window and sfa_session_lengths report W, sfa_session_query_span ends at event skip + W - 1, and status bit 4 marks
 * every call that swept a slot again: every change of W after the first.  State and rows depend on the samples received, not
 * on how they were cut into calls.  Poisoning, full and end of read are as on any raw session.  Under a doubling list
 * (norm, 2 norm, ..., q = norm x 2^m) a read is swept over 2 q - norm events in all.
 * A resweep session accepts every context a session accepts, and SFA_RNA without SFA_INV as well (still not SFA_DTW, not group
 * contexts).  It is raw mode only: sfa_session_extend on it is SFA_EINVAL before and after sfa_session_raw_config -- the caller's
 * events are not kept, so nothing could be swept again.  sfa_session_raw_config, sfa_session_raw_recalibrate, sfa_session_reset,
 * sfa_session_events, sfa_session_query_span and sfa_session_row work as on any raw session. */
int sfa_session_raw_config(sfa_session_t *s, int32_t skip_events, int32_t norm_events, int32_t query_events);

typedef struct {
    int64_t n_samples; /* samples the slot has received since its last reset */
    int64_t n_events;  /* final events (at most skip + query) */
    int64_t q_events;  /* query events swept: the length of the query out[i] is the row of */
    float norm_mean, norm_sd; /* the slot's normalisation, 0 before calibration */
    int32_t status;    /* bit 0 calibrated, bit 1 full, bit 2 ended (end of read seen), bit 3 poisoned, bit 4 (of this call only):
                          the slot was recalibrated and events an earlier call had swept were swept again */
    int32_t norm_window; /* W: norm_mean and norm_sd span final events [skip, skip + W); 0 before calibration */
} sfa_session_raw_info_t;

/* Recalibration: let a slot's normalisation window grow with its read instead of freezing it at norm events.
 * With q_avail = min(n_events - skip, query) query events available, the window W a slot has after a call is
 *   q_avail                        with SFA_RECAL_AT_END, once its end of read has been seen, when 25 <= q_avail < query -- the
 *                                  window the batch path gives a read that is too short (normalise_single, src/sigfish.c:450-461)
 *   the largest at[k] <= q_avail   otherwise, if there is one
 *   norm                           otherwise, if q_avail >= norm
 *   0                              otherwise: not calibrated
 * W never shrinks.  When a call leaves a slot with another W than its normalisation spans, the device computes mean and sd over
 * [skip, skip + W) (sfa_znormalise's arithmetic, as at the first calibration), rewrites the slot's whole query and sweeps it
 * again from event 0 inside that call -- a first chunk, which overwrites the carried row; a call that passes several points takes
 * the last.  So after ANY call out[i] is, bit for bit, sfa_align_batch's row for the slot's q_avail query events normalised over
 * [skip, skip + W), and state and rows depend on the samples a slot has received, not on how they were cut into calls.  Under a
 * doubling list (norm, 2 norm, 4 norm, ..., query) a read is swept at most twice.
 * Allowed on a raw-mode session while every slot is empty; needs norm < at[0] < ... < at[n_at - 1] <= query and n_at <= 32;
 * unknown flags, a bad list, a session that is not in raw mode or a slot in use are SFA_EINVAL.  n_at = 0 with flags = 0
 * switches it off (at may be NULL then), and so does sfa_session_raw_config. */
#define SFA_RECAL_AT_END 0x1
int sfa_session_raw_recalibrate(sfa_session_t *s, const int32_t *at, int32_t n_at, uint32_t flags);

/* Append raw[raw_off[i] .. raw_off[i+1]) to slot slot[i], i < n.  scaling[3*i..]: digitisation, offset, range as for sfa_align_raw;
 * the triple is latched by a slot's first chunk after a reset, another one later is SFA_EINVAL.  end_of_read (may be NULL):
 * end_of_read[i] != 0 runs the detector's finish step for the slot behind the chunk's samples (the chunk may be empty): the
 * remaining positions are walked as the batch detector walks them and the last event runs to the end of the signal; the slot
 * then takes no samples until it is reset (SFA_EINVAL).  out[i]: valid = 0 before calibration; afterwards, bit for bit, the row
 * sfa_align_batch gives for the slot's normalised query so far (with SFA_SESSION_NO_START as for sfa_session_extend).  Slot range
 * and duplicates as for sfa_session_extend; SFA_ERANGE beyond 2^30 samples per slot or per call.  Blocking.  sfa_get_profile
 * afterwards reports events_ms (the detector) and normalise_ms beside fill_ms; total_ms includes them. */
int sfa_session_extend_raw(sfa_session_t *s, const int32_t *slot, const int16_t *raw, const int64_t *raw_off, const double *scaling,
                           const uint8_t *end_of_read, int32_t n, sfa_result_t *out, sfa_session_raw_info_t *info);

/* The slot's final events [first, first + cap) (means in pA, `start` in samples since the reset) copied to out; returns the
 * number of final events the slot has, or < 0. */
int64_t sfa_session_events(sfa_session_t *s, int32_t slot, int64_t first, sfa_event_t *out, int64_t cap);

/* For slot[i], i < n, of a raw-mode session: start_raw[i] = start of final event `skip`, end_raw[i] = start + length of the last
 * query event swept (event skip + q_events - 1), in samples since the slot's reset; both 0 for a slot that is not calibrated.
 * These are the start_raw_idx / end_raw_idx sfa_paf_row takes (the sum is start + (uint64_t)length; the batch path adds in fp32,
 * the same number below 2^24 samples).  One gather on the device, one copy back: a tick's decided slots cost one call, where
 * sfa_session_events is a copy per slot and per end.  Blocking, on the context's stream.
 * SFA_EINVAL: not a raw-mode session, slot out of range. */
int sfa_session_query_span(sfa_session_t *s, const int32_t *slot, int32_t n, uint64_t *start_raw, uint64_t *end_raw);

/* Device memory raw mode adds to sfa_session_bytes: per slot an event table of (skip + query) x 24 bytes, the query of
 * query x 4 bytes and 592 bytes of detector state (the slot's window length, 4 bytes in a side array, counts as bookkeeping).
 * Host arithmetic; negative (an SFA_E* code) for n_slots <= 0, skip < 0,
 * query <= 0 or a product beyond 2^63. */
int64_t sfa_session_raw_bytes(int32_t n_slots, int32_t skip_events, int32_t query_events);

/* ---- automatic query start in a raw session: the RNA "-p -1" of sfa_align_raw, found while the read streams ----------------
 * The adaptor segmenter of detect_query_start is not causal (its threshold is taken over the whole signal), so a session has a
 * rule of its own, stated on samples; state depends on the samples a slot has received, never on how they were cut into calls.
 *   target(N)   what detect_query_start computes before it looks at events, applied to the slot's first N samples: polya.y + ad.y,
 *               a sample index, or -1 when either segmenter fails (sfa_auto_start_target; needs N > 2000).
 *   points      every N_k = k * every_samples <= max_samples, counted from the slot's first sample after its reset
 *               (every_samples = 0: none), and one FINAL point at min(samples received, max_samples), taken when the slot's end of
 *               read is seen or when it has received max_samples samples, whichever comes first.  A call that carries a slot
 *               past several points evaluates them in ascending order, each on its own prefix.
 *   freezing    the target is frozen at the first point with target(N_k) >= 0; later points are not evaluated.  (A poly-A stretch
 *               still open at N_k gives -1, so a frozen target lies in front of N_k.)
 *   skip        the index of the first final event whose start >= target, resolved in the call in which that event becomes final.
 *               Until then the slot has no query: q_events = 0, not calibrated.
 *   failure     the final point gives -1; or the read ends with no event at or behind the frozen target; or the resolved skip
 *               is beyond the largest allowed.  The slot then takes skip = 50, the reference's fallback, and reports why.
 * After that everything is the rule of the raw session with the slot's own skip: windows, SFA_RECAL_AT_END and resweep unchanged,
 * "full" is n_events >= skip + query; the detector stops at the table's capacity only, so n_events may run to max skip + query.
 * With every_samples = 0 and max_samples >= the read's length the only point is the whole read: target, skip and the fallback
 * are those of sfa_align_raw(prefix_size = -1), and with norm = query and SFA_RECAL_AT_END so is the row after the end of read.
 *
 * sfa_session_raw_auto_start: allowed on a raw-mode session created with SFA_SESSION_RESWEEP, on an SFA_RNA context without
 * SFA_END / SFA_INV, while every slot is empty.  The skip_events given to sfa_session_raw_config becomes the LARGEST skip a slot
 * may resolve (it stays the table size: skip + query records) and must be >= 50.  max_samples <= 2^20; max_samples = 0 switches
 * the feature off, and so does sfa_session_raw_config.  flags must be 0.  Everything else is SFA_EINVAL.  The segmenter constants
 * follow the context's pore (sfa_set_pore), as for sfa_align_raw. */
int sfa_session_raw_auto_start(sfa_session_t *s, int32_t every_samples, int32_t max_samples, uint32_t flags);

#define SFA_AUTO_PENDING 0     /* no skip yet (a target may be frozen already) */
#define SFA_AUTO_RESOLVED 1    /* skip is the first event at or behind the target */
#define SFA_AUTO_NO_TARGET 2   /* failed: the final point gave no target; skip = 50 */
#define SFA_AUTO_NO_EVENT 3    /* failed: the read ended with no event at or behind the target; skip = 50 */
#define SFA_AUTO_BEYOND_MAX 4  /* failed: the event lies beyond the largest skip; skip = 50 */
#define SFA_AUTO_AT_FINAL 16   /* (bit) frozen_at is the slot's final point */
typedef struct {
    int64_t target;    /* the frozen target sample, -1 before (and after a failure without one) */
    int64_t frozen_at; /* the point N_k at which the target was frozen, or the final point that gave none; 0 before */
    int32_t skip;      /* the slot's skip, -1 while unresolved */
    int32_t status;    /* SFA_AUTO_* in the low four bits | SFA_AUTO_AT_FINAL */
} sfa_session_auto_t;

/* The automatic start of slot[i], i < n, as the last call left it (host memory, no device work).  SFA_EINVAL on a session without
 * the feature or a slot out of range. */
int sfa_session_auto_start(sfa_session_t *s, const int32_t *slot, int32_t n, sfa_session_auto_t *out);

/* Device time, in ms, that retention and evaluation (the two kernels the feature adds in front of the normaliser) took in the
 * session's last sfa_session_extend_raw call, from events on the context's stream; sfa_profile_t.normalise_ms of that call
 * includes it.  0 before the first call, -1 on a session without the feature. */
double sfa_session_auto_ms(sfa_session_t *s);

/* Device memory the feature adds: per slot max_samples x 2 bytes of retained samples, 16 bytes of state, and (max_samples + 1)
 * x 4 bytes of prefix sums for a call in which every slot has a pending point (the scratch grows to the largest such call).
 * Host arithmetic; negative for n_slots <= 0, max_samples <= 0 or > 2^20. */
int64_t sfa_session_auto_bytes(int32_t n_slots, int32_t max_samples);

/* align_db() shaped entry: per-read event tables exactly as db_t holds them (src/sigfish.h:177-178):
 * events[i] -> sfa_event_t array of read i, qstart[i]/qend[i] the window chosen by normalise_single
 * (src/sigfish.c:479-480); reads with n_events[i]==0 are skipped.  The window means are gathered out of the 24-byte event
 * records into page-locked memory (on a few threads once the batch is large) and uploaded from there. */
int sfa_align_events(sfa_ctx_t *ctx, const sfa_event_t *const *events, const int64_t *n_events,
                     const int64_t *qstart, const int64_t *qend, int32_t n_reads, sfa_result_t *out);

/* Options (all optional; rows never depend on them -- every setting is held to the same parity tests).  15 keys:
 *   planner
 *     "lane_widening"         0 = auto by batch size (default); 1 / 2 / 4 = fixed: rows per lane / w and lanes per read * w -- the
 *                             small-batch latency shapes
 *     "widen_below"           auto mode widens x4 when a batch has fewer wave-tasks per SIMD than this (default 5; a caller with
 *                             several batches in flight per device lowers it)
 *     "column_segments"       0 = auto (small batches cut every (contig,strand) sweep into up to 64 verified segments), 1 = off,
 *                             2..64 = that many
 *     "segment_warm_windows"  query lengths a segment starts early (default 4)
 *     "waves_per_simd"        1..8, occupancy target used when splitting the contig list into chunks (default 6)
 *     "min_slice_reads"       a batch whose checkpoints would not fit the budget at the shortest interval is cut into slices of at
 *                             least this many reads, run back to back (default 65536)
 *   pass 1 -> pass 2 hand-over
 *     "lds_ckpt"              1 = default: where every shape of the batch has <= 16 rows per lane (queries up to 256 events) the fill
 *                             keeps every read's last two snapshots in LDS, taken where the read's own windows end, and writes the
 *                             older one to HBM only when a window becomes the read's best so far (pass 2 then starts one own window
 *                             in front of it), plus a sparse store every 32768 steps for pass 2 to back off to (--dtw-std: the sparse store
 *                             alone); 2 = the same whatever the batch size and up to 1024 events at 16 rows per lane; 0 = every
 *                             snapshot to HBM.  Shapes with 32 rows per lane always keep their snapshots in HBM.
 *     "fused_trace"           1 = default: pass 2 runs inside the fill launch (tickets) when the launch has more wave-tasks than the
 *                             device has wave slots; 2 = always; 0 = always as its own launch
 *     "ckpt_interval"         0 = auto, else a power of two >= 4: snapshots of pass 1 in HBM every that many steps
 *     "ckpt_budget_bytes"     HBM the snapshots of one batch may take (default 32 GiB)
 *     "trace_margin"          -1 = auto: pass 2 starts a query length (+ lanes) in front of the winning window -- on the HBM-snapshot
 *                             route as far as 99.9 % of the PREVIOUS batch's alignments spanned, rounded up to the next sixteenth of
 *                             the query, + 1/16 query + lanes + 16; a read whose path is longer backs off one snapshot; >= 0: that
 *                             many steps.  On the LDS route the head start follows from the windows (one own window less the lane
 *                             skew: sfa_profile_t.trace_margin reports the longest read's) and the option only bounds what pass 2
 *                             asks of the sparse store when it backs off
 *   launch
 *     "prio_unit"             columns per level of the fill's longest-remaining-first issue priority in the tail of a launch
 *                             (default 2048; 0 = off)
 *     "spin_limit_ms"         default 20000: the longest a wave of a launch waits for another wave of the same launch -- pass 2 for
 *                             its quad's fill tasks, a row strip for the strip above -- before the batch fails with SFA_EKERNEL;
 *                             floors apply (about five times the longest fill task; the strips' pipeline depth)
 *   output
 *     "secondary"             0..4 (default 0): secondary mappings per read, returned by sfa_secondary_rows; > 0 takes the plain
 *                             two-pass route (HBM snapshots, no column segments, pass 2 as its own launches).  Rows do not change
 *     "secondary_strips"      0 (default) or 1, with an effect only while "secondary" is 1..4: reads of more than SFA_MAX_QUERY events
 *                             have secondaries too.  Pass 1 of the row strips then runs as a kernel of its own that keeps each (read,
 *                             contig, strand)'s list of its 5 best windows, a merge ranks them, and pass 2 runs once more per rank.
 *                             Primaries do not change; 0 launches what it always did and leaves those reads' slots at valid = 0
 *     "map_scratch_bytes"     HBM the packed moves of one slice of rows may take in sfa_event_maps (default 2 GiB); rows are processed in
 *                             slices that fit, a row that does not fit alone goes to the host routine
 *     "map_strips"            0 (default) or 1: sfa_event_maps and sfa_session_event_maps run a row of more than SFA_MAX_QUERY events on
 *                             the device, in strips of SFA_MAX_QUERY query rows (ceil(events / 2048) strips of (m + 63) * 512 bytes of
 *                             moves for a band of m columns, plus two hand-over rows of m floats: all of it counts against
 *                             "map_scratch_bytes"), instead of on the host inside the call.  Same maps; 0 launches what it always did
 *   raw-signal path
 *     "ev_parallel"           bit 0: wave-per-read prefix sums for every read whose sums are provably exact in any order (the
 *                             sequential kernel for the rest); bit 1: chunk-parallel peak picker accepted where it is certified
 *                             to equal the sequential one; default 3
 * Test hooks, refused unless SFA_TEST_HOOKS=1 is in the environment: "debug_drop_quad" / "debug_drop_strip" (the producer with
 * this index never signals; every batch then fails with SFA_EKERNEL after the wait limit; -1 = off). */
int sfa_set_option(sfa_ctx_t *ctx, const char *key, int64_t value);

/* Pore chemistry, the reference's opt.pore_flag: 0 R9 (default), 1 R10, 2 RNA004; applies to every shard.  It changes rows:
 * the RNA automatic query start (prefix_size < 0) looks for an adaptor of >= 500 samples below mean - 0.7 sd on RNA004,
 * of >= 2000 samples below mean - 0.5 sd otherwise (src/jnn.h).  SFA_EINVAL outside 0..2. */
int sfa_set_pore(sfa_ctx_t *ctx, int pore);

/* Plan a batch without running it: how reads would be grouped.  slot_of_read[n_reads] (may be NULL) receives
 * quad*4+slot per read or -1 for skipped reads; job_len[n_jobs] are the (contig,strand) lengths in processing
 * order.  ckpt_interval / ckpt_budget_bytes / lane_widening as in sfa_set_option (0 = defaults; the device is
 * assumed to have 1024 SIMDs). */
int sfa_plan_batch(const int64_t *q_off, int32_t n_reads, const int32_t *job_len, int32_t n_jobs, int64_t ckpt_interval,
                   int64_t ckpt_budget_bytes, int32_t lane_widening, int32_t *slot_of_read, sfa_plan_info_t *info);

/* Block until everything enqueued on the context stream has finished. */
int sfa_sync(sfa_ctx_t *ctx);

/* Timing of the most recent align call (valid after it completed / after sfa_sync). */
int sfa_get_profile(sfa_ctx_t *ctx, sfa_profile_t *prof);

/* The HIP stream (hipStream_t) the context enqueues on, as an opaque pointer. */
void *sfa_stream(sfa_ctx_t *ctx);

void sfa_destroy(sfa_ctx_t *ctx);

const char *sfa_last_error(void);
const char *sfa_version(void);
/* Identity of the device code this library was built from (hash of the kernel and launch sources): profiles/ files are
 * stamped with it, so that numbers measured on one build are never quoted for another. */
const char *sfa_build_id(void);

/* ---- host-side helpers on the same path (no GPU needed) ------------------------------------------------ */

/* Reference event model from sequences (gen_ref, src/genref.c:86-241), one record at a time.
 * level_mean[4^k]: k-mer model means.  fwd/rev must hold (len+1-k) floats (rev may be NULL for RNA).
 * Returns the k-mer count ref_len (or <0 on error) and stores ref_st_offset. */
int32_t sfa_gen_ref_record(const char *seq, int32_t len, const float *level_mean, uint32_t k, uint32_t flag,
                           int32_t query_size, float *fwd, float *rev, int32_t *st_offset);

/* z-normalisation used for both queries and reference arrays (src/sigfish.c:483-502, src/genref.c:23-47). */
void sfa_znormalise(float *v, uint64_t n);

/* One PAF line for a result row (paf_str, src/sigfish.c:628-660).  Returns bytes written (excluding NUL),
 * or a negative value if cap is too small. */
int sfa_paf_row(char *buf, size_t cap, const sfa_result_t *r, const char *read_id, const char *rname,
                uint64_t start_raw_idx, uint64_t end_raw_idx, uint64_t query_size, uint64_t len_raw_signal,
                uint64_t rlength);
/* The same with the type tag: tp = 'P' (what sfa_paf_row writes) or 'S' for a row of sfa_secondary_rows. */
int sfa_paf_row_ex(char *buf, size_t cap, const sfa_result_t *r, const char *read_id, const char *rname,
                   uint64_t start_raw_idx, uint64_t end_raw_idx, uint64_t query_size, uint64_t len_raw_signal,
                   uint64_t rlength, char tp);

/* ---- raw signal in, result rows out: the pre-DP stages on the GPU as well --------------------------------- */

/* What the output writer needs besides the result row (aln_to_str, src/sigfish.c:796-826). */
typedef struct {
    int64_t n_events;       /* events detected in the read (0: read dropped) */
    int64_t qstart, qend;   /* query window in events (src/sigfish.c:479-480) */
    uint64_t start_raw_idx; /* event[qstart].start */
    uint64_t end_raw_idx;   /* event[qend-1].start + length */
    int32_t status;         /* bit 0: too short (kept), bit 1: ignored (dropped), bit 2: automatic query start failed (the
                               window starts at event 50; the reference's prefix_fail, src/sigfish.c:438-446) */
    int32_t pad;
} sfa_query_info_t;

/* process_db() for a whole batch on the device (src/sigfish.c:1018-1047 minus parsing): raw ADC samples -> pA ->
 * event detection -> query window -> z-normalisation -> alignment.  raw: concatenated int16 samples, raw_off[n+1];
 * scaling[3*i..]: digitisation, offset, range of read i (slow5 record fields).  prefix_size < 0 is the RNA automatic query
 * start ("-p -1", detect_query_start, src/sigfish.c:380-422 + src/jnn.c), also on the device: the window starts at the
 * first event behind the poly-A tail, or at event 50 where none is found (status bit 2).  It needs an SFA_RNA context
 * without SFA_END and SFA_INV (else SFA_EINVAL), and follows the context's pore (sfa_set_pore).
 * rows[n] and info[n] are written in input order.  Blocking. */
int sfa_align_raw(sfa_ctx_t *ctx, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n_reads,
                  int32_t prefix_size, int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info);

/* Same, and the event table of every read's query window comes back as well: query_events[i * query_size + e], e <
 * info[i].qend - info[i].qstart, holds event qstart + e of read i with its mean z-normalised -- what sfa_sam_row needs
 * (pass it with qstart = 0, qend = the window length).  query_events may be NULL (then identical to sfa_align_raw). */
int sfa_align_raw_ex(sfa_ctx_t *ctx, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n_reads,
                  int32_t prefix_size, int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_event_t *query_events);

/* ---- BLOW5 records in, result rows out: the record decoder on the GPU as well ------------------------------ */

/* What the output writer needs from a record besides its alignment (slow5_rec_t fields, slow5lib/include/slow5/slow5.h). */
typedef struct {
    char read_id[128];     /* NUL terminated */
    int32_t id_len;
    int32_t pad;
    int64_t n_samples;     /* len_raw_signal */
    double digitisation, offset, range;
    int64_t record_bytes;  /* on-disk size of the record (the reference's -B accounting, src/sigfish.c:304) */
} sfa_read_head_t;

/* load_db()'s records straight to the device (src/sigfish.c:274-314 hands them to parse_single, 317-328, on host threads):
 * records: the BLOW5 records of a batch back to back WITHOUT their u64 size prefixes, rec_off[n+1] their offsets;
 * record_zlib / signal_svb: the file's compression methods: record_zlib is the file's record_press -- SFA_PRESS_NONE (0),
 * SFA_PRESS_ZLIB (1) or SFA_PRESS_ZSTD (2) -- and signal_svb says signal_press == svb-zd.  Every record is decompressed
 * (own DEFLATE decoder or own zstd decoder, one lane per record), its primary fields are parsed and its signal decoded
 * (StreamVByte zig-zag deltas, one wave per record) on the device; the path of sfa_align_raw_ex continues from there.
 * heads[n] receives the fields the output needs.  A record the device decoder declines (malformed, longer read id than
 * sfa_read_head_t holds, decompressing to more than 4x its size + 4 KB, signal stream longer or shorter than its keys say) sends
 * the batch through the library's host reader instead -- same results, counted in sfa_profile_t.blow5_fallbacks; a record the
 * host reader rejects as well is SFA_EINVAL naming it.  Other arguments as for sfa_align_raw_ex (prefix_size < 0 included). */
#define SFA_PRESS_NONE 0 /* record_zlib: the records are not compressed */
#define SFA_PRESS_ZLIB 1 /* ... every record is a zlib stream */
#define SFA_PRESS_ZSTD 2 /* ... every record is a zstd frame */
int sfa_align_blow5(sfa_ctx_t *ctx, const uint8_t *records, const int64_t *rec_off, int32_t n_reads, int32_t record_zlib,
                    int32_t signal_svb, int32_t prefix_size, int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info,
                    sfa_read_head_t *heads, sfa_event_t *query_events);

/* The device-side zstd decoder on its own (tests): n zstd records in[in_off[i]..in_off[i+1]) -> out[out_off[i]..),
 * out_len[i] = bytes produced or -1 (malformed, or larger than its slot).  Single-device context. */
int sfa_zstd_device(sfa_ctx_t *ctx, const uint8_t *in, const int64_t *in_off, int32_t n, uint8_t *out, const int64_t *out_off,
                    int32_t *out_len);

/* The device-side DEFLATE decoder on its own (tests): n zlib streams in[in_off[i]..in_off[i+1]) -> out[out_off[i]..),
 * out_len[i] = bytes produced or -1 (malformed, or larger than its slot).  Single-device context. */
int sfa_inflate_zlib_device(sfa_ctx_t *ctx, const uint8_t *in, const int64_t *in_off, int32_t n, uint8_t *out, const int64_t *out_off,
                            int32_t *out_len);

/* The device-side record decoder on its own (tests): the stages sfa_align_blow5 runs before the alignment -- inflate, field
 * parser, signal decoder -- and what they left on the device, with NO host reader behind them.  records, rec_off, n, record_zlib,
 * signal_svb as for sfa_align_blow5.  status[n]: 0 decoded, or why the device declined the record (one declined record is what
 * sends a batch of sfa_align_blow5 to the host reader).  raw_off[n+1]: where every record's samples lie in samples[]; a record
 * with SFA_BLOW5_INFLATE or SFA_BLOW5_FIELDS counts no samples and gets a zeroed head (record_bytes apart), one with
 * SFA_BLOW5_STREAM keeps its head and its n_samples places, whose contents are undefined; all others are decoded whatever their
 * neighbours are.  samples: room for `capacity` int16; SFA_ERANGE when raw_off[n] exceeds it (status, heads and raw_off are
 * written by then).  Single-device context. */
#define SFA_BLOW5_INFLATE 1 /* the record does not decompress (malformed, truncated, or more than 4x its size + 4 KB) */
#define SFA_BLOW5_FIELDS 2  /* the primary fields: payload too short for them or for the signal they announce, read id too long */
#define SFA_BLOW5_STREAM 3  /* svb-zd: the data stream is longer or shorter than its keys say */
int sfa_decode_blow5_device(sfa_ctx_t *ctx, const uint8_t *records, const int64_t *rec_off, int32_t n, int32_t record_zlib,
                            int32_t signal_svb, int32_t *status, sfa_read_head_t *heads, int64_t *raw_off, int16_t *samples,
                            int64_t capacity);

/* The event detection of sfa_align_raw on its own (tests): every read's WHOLE event table instead of the query window, means in
 * pA (not normalised).  raw, raw_off[n_reads+1], scaling as for sfa_align_raw; the context's flag selects the DNA or RNA detector
 * and option "ev_parallel" is honoured.  Read i owns events[raw_off[i] + 2 * i ...], room for its samples + 2 records (the
 * device's own capacity rule), of which the first n_events[i] are written.  route[i]: bit 0 = the sequential prefix-sum kernel
 * summed this read, bit 1 = the sequential peak picker walked it (clear: the wave-per-read kernel certified its own result).
 * t_short / t_long: NULL, or raw_off[n_reads] floats each, the two t-statistics of every sample.  Single-device context. */
int sfa_detect_events_device(sfa_ctx_t *ctx, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n_reads,
                             sfa_event_t *events, int32_t *n_events, int32_t *route, float *t_short, float *t_long);

/* Page-locked host memory for the buffers handed to sfa_align_raw / sfa_align_batch (uploads from pageable memory
 * run at a fraction of the PCIe rate).  Plain malloc-style pair; NULL on failure. */
void *sfa_pinned_alloc(size_t bytes);
void sfa_pinned_free(void *p);

/* ---- host pre-DP stages and readers (no GPU needed) ----------------------------- */

/* event_single (src/sigfish.c:330-378): raw ADC samples -> pA -> events (getevents, src/events.c:557-577).
 * Writes at most cap events to out; returns the number of events detected (call again with a larger buffer if
 * the return value exceeds cap), or <0 on error. */
int64_t sfa_detect_events(const int16_t *raw, int64_t n_raw, double digitisation, double offset, double range, int rna,
                          sfa_event_t *out, int64_t cap);

/* The same detector fed a read in chunks (a sequencing channel delivers its samples a few hundred at a time).  With N samples
 * seen and N >= 2 w_long (w_long = 6 DNA / 14 RNA) both t-statistics of every position j <= N - w_long are already what the whole
 * read will give, and the peak picker is causal: so a push walks the picker over exactly those positions, and every event whose
 * closing peak has fired is FINAL -- equal in all four fields, bit for bit, to the same event of sfa_detect_events over the
 * complete read.  Nothing is withheld and nothing is processed while N < 2 w_long.  sfa_event_stream_finish walks the remaining
 * positions as the batch code does and closes the last event at the end of the signal: everything push returned plus what
 * finish returns IS the table of sfa_detect_events.  `start` counts samples since creation.  The state is a constant number of
 * words (a ring of the last 2 w_long + 1 prefix sums, the two detectors, the sums at their candidate peaks and at the open
 * event's start); it does not grow with the read.
 * push / finish write the events that became final to out (at most cap) and return their number; when that exceeds cap nothing
 * is consumed -- call again with a larger buffer (push: and the same samples).  SFA_EINVAL: null arguments, samples after finish,
 * a second finish. */
typedef struct sfa_event_stream sfa_event_stream_t;
sfa_event_stream_t *sfa_event_stream_create(double digitisation, double offset, double range, int rna);
int64_t sfa_event_stream_push(sfa_event_stream_t *es, const int16_t *raw, int64_t n, sfa_event_t *out, int64_t cap);
int64_t sfa_event_stream_finish(sfa_event_stream_t *es, sfa_event_t *out, int64_t cap);
void sfa_event_stream_destroy(sfa_event_stream_t *es);

/* normalise_single (src/sigfish.c:424-505): choose the query window [qstart,qend) from -p/-q/--from-end
 * (prefix_size < 0: RNA adaptor/poly-A auto detection, src/sigfish.c:380-422 + src/jnn.c) and z-normalise those
 * event means in place.  Returns 1 if the read is kept, 0 if the reference would drop it (et.n = 0). */
int sfa_select_query(sfa_event_t *events, int64_t n_events, const int16_t *raw, int64_t n_raw, double digitisation,
                     double offset, double range, int32_t prefix_size, int32_t query_size, uint32_t flag, int pore,
                     int64_t *qstart, int64_t *qend);

/* detect_query_start (src/sigfish.c:380-422): the RNA automatic query start of one read -- the first event whose start lies at
 * or behind the end of the poly-A tail that follows the adaptor -- or -1 when the adaptor or the tail is not found (callers
 * then start at event 50).  events: the read's event table (sfa_detect_events); pore as for sfa_set_pore. */
int64_t sfa_detect_query_start(const int16_t *raw, int64_t n_raw, double digitisation, double offset, double range,
                               const sfa_event_t *events, int64_t n_events, int pore);

/* What detect_query_start computes before it looks at events, for the first n samples of a read: the sample index behind the
 * poly-A tail that follows the adaptor (polya.y + ad.y), or -1 when the adaptor or the tail is not found (n <= 2000 among the
 * causes).  The host twin of a session's automatic query start (sfa_session_raw_auto_start). */
int64_t sfa_auto_start_target(const int16_t *raw, int64_t n, double digitisation, double offset, double range, int pore);

/* One SAM line for a result row (sam_str, src/sigfish.c:770-794, with path_to_map 530-571 and the "ss" string of
 * r2qevent_map_to_ss 663-768).  The warp path of the winner is rebuilt on the host from the band between its
 * start and end columns.  events/qstart/qend: the read's event table and query window as for sfa_align_events
 * (means z-normalised); ref_array: the winner's (contig,strand) array -- forward[rid] for '+', reverse[rid] for
 * '-' -- of ref_len floats; ref_st_offset as given to sfa_init.  Returns bytes written or <0. */
int sfa_sam_row(char *buf, size_t cap, const sfa_result_t *r, const char *read_id, const char *rname,
                const sfa_event_t *events, int64_t qstart, int64_t qend, const float *ref_array, int32_t ref_len,
                int32_t ref_st_offset, uint32_t flag);
/* The same; secondary != 0 sets FLAG bit 256 (a row of sfa_secondary_rows). */
int sfa_sam_row_ex(char *buf, size_t cap, const sfa_result_t *r, const char *read_id, const char *rname,
                   const sfa_event_t *events, int64_t qstart, int64_t qend, const float *ref_array, int32_t ref_len,
                   int32_t ref_st_offset, uint32_t flag, int secondary);

/* The same line from a map instead of a path: pairs[2 * n_pairs] as sfa_r2qevent_map or sfa_event_maps return it for the row.
 * Host only, no reference array needed.  SFA_EINVAL also for a map whose indices leave the query window, and for a map the ss
 * string cannot express: with SFA_RNA every index is mirrored about the last column's stop, so a map whose last column is blank
 * (-1/-1: the path entered it without advancing in the query, common under SFA_DTW) has no record -- r2qevent_map_to_ss asserts
 * there (src/sigfish.c:668-669).  sfa_sam_row and sfa_sam_row_ex format through this function and refuse the same rows. */
int sfa_sam_row_from_map(char *buf, size_t cap, const sfa_result_t *r, const char *read_id, const char *rname,
                         const sfa_event_t *events, int64_t qstart, int64_t qend, const int32_t *pairs, int32_t n_pairs,
                         uint32_t flag, int secondary);

/* aln_t.r2qevent_map for a result row (path_to_map, src/sigfish.c:530-571, as update_aln stores it at 610-613): what the
 * reference's own sam_str / r2qevent_map_to_ss (src/sigfish.c:663-794) consume.  The winner's warp path is rebuilt on the
 * host from the band between its start and end columns, exactly as for sfa_sam_row; arguments as there.
 * pairs[2*i], pairs[2*i+1] = start, stop (query event indices relative to qstart, in DP order) for reference column
 * pos_st + i -- the memory layout of index_pair_t[] (src/sigfish.h:141-144), so a C host may pass its own array.
 * Returns r2qevent_size = pos_end - pos_st + 1 (also when pairs is NULL: size query), SFA_ERANGE if cap_pairs (in pairs)
 * is smaller than that, SFA_EINVAL for an unaligned row. */
int32_t sfa_r2qevent_map(const sfa_result_t *r, const sfa_event_t *events, int64_t qstart, int64_t qend, const float *ref_array,
                         int32_t ref_len, int32_t ref_st_offset, uint32_t flag, int32_t *pairs, int32_t cap_pairs);

/* read_model (src/model.c:38-131): text k-mer model -> level_mean[4^k] (levels must hold 262144 floats).  Accepts and refuses what
 * the reference does; rows it would only have logged as corrupted (src/model.c:98-100) are counted like it counts them and listed
 * in sfa_last_error() after a successful return (empty string: none). */
int sfa_read_kmer_model(const char *path, float *levels, uint32_t *k);

/* Sequential S/BLOW5 reader, the subset of slow5lib the path uses (slow5_open, src/sigfish.c:110): BLOW5 (zlib / svb-zd /
 * uncompressed) and its text twin SLOW5 ASCII, told apart by content (slow5lib: by the extension).  Numbers in a text file are
 * accepted as slow5lib accepts them (slow5_misc.c:103-156); auxiliary columns are counted, not interpreted. */
typedef struct sfa_blow5 sfa_blow5_t;
sfa_blow5_t *sfa_blow5_open(const char *path);            /* NULL on failure, see sfa_last_error() */
const char *sfa_blow5_attr(sfa_blow5_t *f, const char *key); /* header attribute of read group 0 or NULL */
/* 1: a record was read, 0: end of file, <0: error.  Pointers stay valid until the next call on f.
 * meta = {digitisation, offset, range, sampling_rate}. */
int sfa_blow5_next(sfa_blow5_t *f, const char **read_id, double meta[4], const int16_t **raw, int64_t *n_raw);
void sfa_blow5_close(sfa_blow5_t *f);
/* One rank's part of a read-sharded run (replaces the whole-file loop of src/dtw_main.c:299-326 by G loops over disjoint parts;
 * records are framed by their u64 size prefixes only, slow5lib/src/slow5.c:3218-3266, so a part is found by walking them).
 * Call after sfa_blow5_open and before the first sfa_blow5_next; past the selection sfa_blow5_next returns 0.
 *   sfa_blow5_select_shard    the records whose size prefix starts in the r-th of G equal byte slices of the record region:
 *                             the G shards are every record exactly once, in file order (regular files only)
 *   sfa_blow5_select_records  records [first, first + count) by position in the file (count < 0: to the end) */
int sfa_blow5_select_shard(sfa_blow5_t *f, int32_t r, int32_t G);
int sfa_blow5_select_records(sfa_blow5_t *f, int64_t first, int64_t count);

/* Free and total memory of a device in bytes (hipMemGetInfo), for callers sizing their batches. */
int sfa_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* The record decompressor of the BLOW5 reader on its own: inflates the zlib stream in[0..n) into out[0..cap) with the
 * library's own DEFLATE decoder and returns the number of bytes produced, SFA_ERANGE when cap is too small, SFA_EINVAL
 * when the decoder declines the stream (the reader then falls back to zlib's inflate). */
int64_t sfa_inflate_zlib(const uint8_t *in, size_t n, uint8_t *out, size_t cap);

/* The same for TWO streams decoded side by side by the calling thread (how the reader's host threads take records: the symbol
 * loops of the two streams take turns, two dependence chains keep a core busier than one).  len[k] receives what
 * sfa_inflate_zlib would return for stream k -- a stream that is declined does not disturb the other.  Returns SFA_OK, or
 * SFA_EINVAL for null arguments. */
int sfa_inflate_zlib_pair(const uint8_t *in0, size_t n0, const uint8_t *in1, size_t n1, uint8_t *out0, size_t cap0, uint8_t *out1,
                          size_t cap1, int64_t len[2]);

/* The zstd record decompressor of the BLOW5 reader on its own (the library's own decoder, written from RFC 8878: frames back to
 * back, skippable frames, content checksum; no dictionaries): src[0..n) -> dst[0..cap).  Returns the number of bytes produced,
 * or -1 when the frames are malformed or hold more than cap bytes. */
int64_t sfa_zstd_decompress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SIGFISH_AMD_H */
